// rt_update.cpp — rt_update_geometry (include/rt_abi.h): new per-triangle arrays for a built scene, without rt_destroy + rt_create.
//
// Everything that does not follow from the five arrays stays where it is: materials, texture views, the 268 MB texel pool, the tables, the
// analytic primitives, the camera, the stream, the wavefront workspace. What does follow from them is the geometry half of rt_create
// (prepare_geometry on the host: rt_scene_prepare.cpp; upload_geometry on the device: rt_scene.cpp), and the two modes differ in how much of it runs again:
//   RT_UPDATE_REBUILD  all of it, into new buffers beside the live ones; then swap and free. The scene is the one rt_create would build.
//   RT_UPDATE_REFIT    (RT_BUILD_WIDE) the light half on the host as in REBUILD; the scene tree keeps its topology and is refitted in
//                      place on the device (rt_wide_refit.hip), the triangle and shading records are rewritten in place.
// rt_update_geometry_device is the same call for arrays that are in the scene GPU's memory already. What rt_update_geometry does with two host
// loops (the data-dependent refusals, the pick of the lights) one pass on the device does (rt_update_dev.hip); the device build and the refit
// read the caller's arrays where they are; only the builds that read the arrays on the host stage a copy and run the host path.
#include <cstring>

#include "rt_scene_impl.h"
#include "rt_update_dev.h"
#include "rt_wide_refit.h"
#include "wide_grid.h"

namespace {

// The checks of the two entry points, in the order both make them. `fn` names the entry point in the message.
// ... of the struct alone, before the scene is looked at (`device`: the five pointers are device pointers, read by dword loads)
int check_struct(const rt_geometry_update *u, const std::string &fn, bool device) {
    if (!u)
        return rt::fail(RT_ERR_INVALID_ARG, fn + ": null argument");
    if (u->mode != RT_UPDATE_REBUILD && u->mode != RT_UPDATE_REFIT)
        return rt::fail(RT_ERR_INVALID_ARG, fn + ": unknown mode");
    for (uint32_t r : u->reserved)
        if (r)
            return rt::fail(RT_ERR_INVALID_ARG, fn + ": reserved field is not 0");
    if (u->n_triangles && (!u->positions || !u->normals || !u->texcoords || !u->tangents || !u->material_ids))
        return rt::fail(RT_ERR_INVALID_ARG, fn + ": null geometry array");
    if (device)
        for (const void *p : {(const void *)u->positions, (const void *)u->normals, (const void *)u->texcoords, (const void *)u->tangents, (const void *)u->material_ids})
            if ((uintptr_t)p & 3u)
                return rt::fail(RT_ERR_INVALID_ARG, fn + ": misaligned geometry array (device pointers must be 4-byte aligned)");
    return RT_OK;
}
// ... of the scene against the struct
int check_scene(const rt_scene *s, const rt_geometry_update *u, const std::string &fn) {
    if (!s)
        return rt::fail(RT_ERR_INVALID_ARG, fn + ": null scene");
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, fn + ": multi-GPU scenes cannot be updated");
    if (u->n_triangles != s->dev.n_triangles)
        return rt::fail(RT_ERR_INVALID_ARG, fn + ": n_triangles is " + std::to_string(u->n_triangles) + ", the scene has " + std::to_string(s->dev.n_triangles));
    if (s->live_accums)
        return rt::fail(RT_ERR_INVALID_ARG, fn + ": the scene has " + std::to_string(s->live_accums) +
                                                " live accumulator(s), whose sums are of the old geometry: destroy them first");
    return RT_OK;
}
// ... of the arrays' contents: rt_create's host loops (rt::check_geometry_contents) for host arrays, k_update_scan's findings for device arrays:
// the same two refusals in the same order
int refuse_scan_findings(const rt::UpdateScan &scan, const std::string &fn) {
    if (scan.bad_material)
        return rt::refuse_material(fn);
    if (scan.first_non_finite != RT_NONE)
        return rt::refuse_non_finite(fn, scan.first_non_finite);
    return RT_OK;
}
// ... and of the mode against the scene
bool check_mode_ok(const rt_scene *s, const rt_geometry_update *u) { return !(u->mode == RT_UPDATE_REFIT && !(s->prep->build_flags & RT_BUILD_WIDE)); }
int check_mode(const rt_scene *s, const rt_geometry_update *u, const std::string &fn) {
    if (!check_mode_ok(s, u))
        return rt::fail(RT_ERR_UNSUPPORTED, fn + ": RT_UPDATE_REFIT needs a scene built with RT_BUILD_WIDE (a refitted binary tree is "
                                                 "not the reference's topology): use RT_UPDATE_REBUILD");
    return RT_OK;
}

const std::string FN_HOST = "rt_update_geometry", FN_DEVICE = "rt_update_geometry_device";

// what the geometry half reads of a descriptor: the new arrays and how the scene asked to be built
rt_scene_desc geometry_desc(const rt_scene *s, const rt_geometry_update *u) {
    rt_scene_desc d{};
    d.abi_version = RT_ABI_VERSION;
    d.n_triangles = u->n_triangles;
    d.positions = u->positions;
    d.normals = u->normals;
    d.texcoords = u->texcoords;
    d.tangents = u->tangents;
    d.material_ids = u->material_ids;
    d.n_materials = (uint32_t)s->prep->mats.size();
    d.build_flags = s->prep->build_flags;
    d.build = s->prep->build;
    return d;
}

// The new buffers from a prepared geometry half, beside the live ones; then swap and free. `arrays`: see rt::upload_geometry.
int rebuild_from(rt_scene *s, const rt_scene_desc &d, const std::shared_ptr<rt::PreparedGeometry> &G, const rt::DeviceArrays *arrays, const std::string &fn) {
    const rt::PreparedScene &P = *s->prep;
    // a refusal below leaves the scene as it was (`g` frees what was built)
    rt::GeometryOnDevice g;
    int rc = rt::upload_geometry(s, &d, P, *G, g, arrays);
    hipError_t se = rc == RT_OK ? hipDeviceSynchronize() : hipSuccess; // uploads went through the null stream
    if (rc == RT_OK && se != hipSuccess)
        rc = rt::fail(RT_ERR_HIP, fn + ": " + hipGetErrorString(se));
    if (rc != RT_OK)
        return rc;
    rt::install_geometry(s, g); // swaps, then frees the old buffers
    s->geo = G;
    s->refitted = false;
    return RT_OK;
}

int rebuild(rt_scene *s, const rt_scene_desc &d, const std::string &fn) {
    const rt::PreparedScene &P = *s->prep;
    auto G = std::make_shared<rt::PreparedGeometry>();
    rt::prepare_geometry(&d, rt::emissive_materials(P.mats), P.wide_cost_node, P.wide_cost_tri, *G);
    return rebuild_from(s, d, G, nullptr, fn);
}

// The refit proper, from arrays on the device and the light half prepared on the host: `in` has the five arrays and the bounds of their
// vertices, `G` the light tree and its records (null: the light tree, its records and s->geo stay as they are; the caller knows that the
// tree `G` would hold is the live one bit for bit).
int refit_from(rt_scene *s, const std::shared_ptr<rt::PreparedGeometry> &G, const rt::RefitInput &in, const std::string &fn) {
    DevScene &D = s->dev;
    const char *what = "";
    const WideGrid grid = rt::make_wide_grid(in.lo, in.hi);
    if (D.scene.n_wide != 0u && !rt::wide_grid_in_range(grid))
        return rt::fail(RT_ERR_UNSUPPORTED, fn + ": the new extent is outside the 8-wide tree's exponent range (2^-52 .. 2^52)");
    rt::GeometryOnDevice lg; // only its light half is filled: the new tree beside the live one (a failure leaves the stream idle before `lg` frees it)
    if (int rc = G ? rt::upload_light_tree(G->flat[1], G->laux, lg.light_owned, s->stream, lg.lights, lg.light_aux, lg.facts.dev_n_inner[1]) : RT_OK; rc != RT_OK)
        return rc;
    // ---- device, part 2: records and nodes in place (its scratch is allocated first: RT_ERR_OOM still leaves the scene as it was)
    double levels_ms = 0;
    const auto t_refit = std::chrono::steady_clock::now();
    if (hipError_t e = rt::refit_wide_device(in, const_cast<DevTri *>(D.scene.tris), const_cast<DevAttr *>(D.attrs), D.scene.n_tris, const_cast<uint4_pod *>(D.scene.wide),
                                             D.scene.n_units, D.scene.n_wide, grid, s->stream, &what, &levels_ms);
        e != hipSuccess) {
        (void)hipStreamSynchronize(s->stream);
        return rt::hip_fail(e, fn + ": " + what);
    }
    // ---- host: what the launches read of the tree besides the blob
    if (G) {
        D.lights = lg.lights;
        D.light_aux = lg.light_aux;
        s->facts.dev_n_inner[1] = lg.facts.dev_n_inner[1];
        s->light_owned = std::move(lg.light_owned); // frees the old light buffers
    }
    D.scene.grid = grid;
    for (int k = 0; k < 3; ++k)
        rt::sort_bounds_axis(in.lo[k], in.hi[k], D.bounds_lo[k], D.bounds_inv[k]);
    s->refit_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_refit).count();
    s->refit_levels_ms = levels_ms;
    if (G)
        s->geo = G; // (its host_bvh[0] / wide are empty: the tree the wide one was collapsed from no longer describes the scene)
    s->refitted = true;
    ++s->geo_generation; // records rewritten in place: nothing derived from the old ones may be used again
    return RT_OK;
}

int refit(rt_scene *s, const rt_geometry_update *u, const rt_scene_desc &d) {
    const rt::PreparedScene &P = *s->prep;
    if (u->n_triangles == 0)
        return RT_OK;
    // ---- host: the light tree and its records, as in REBUILD (the light set follows the new material ids)
    auto G = std::make_shared<rt::PreparedGeometry>();
    rt::prepare_geometry(&d, rt::emissive_materials(P.mats), P.wide_cost_node, P.wide_cost_tri, *G, /*lights_only=*/true);
    // ---- device, part 1: nothing a render kernel reads is written before the update can no longer be refused
    rt::RefitInput in;
    const char *what = "";
    if (hipError_t e = rt::refit_upload(u, s->stream, &in, &what); e != hipSuccess)
        return rt::hip_fail(e, std::string("rt_update_geometry: ") + what);
    return refit_from(s, G, in, FN_HOST);
}

// ------------------------------------------------------------------------------------------------ arrays that are on the device already
// "device memory of the scene's GPU": first and last byte of each array, by hipPointerGetAttributes (an unregistered host pointer is an error
// or hipMemoryTypeUnregistered, depending on the runtime; pinned host memory is hipMemoryTypeHost; both are refused before any launch)
} // namespace
int rt::check_device_array(const rt_scene *s, const void *p, size_t bytes, const std::string &fn) {
    for (const char *q : {(const char *)p, (const char *)p + bytes - 1}) {
        hipPointerAttribute_t at{};
        const hipError_t e = hipPointerGetAttributes(&at, q);
        if (e != hipSuccess)
            (void)hipGetLastError(); // "not a pointer HIP knows" is an answer, not a failure of the library
        if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != s->device)
            return rt::fail(RT_ERR_INVALID_ARG, fn + ": a geometry array is not device memory of the scene's GPU (device " + std::to_string(s->device) + ")");
    }
    return RT_OK;
}
int rt::check_device_pointers(const rt_scene *s, const rt_geometry_update *u) {
    const size_t n = u->n_triangles;
    const struct {
        const void *p;
        size_t bytes;
    } arrays[5] = {{u->positions, 36 * n}, {u->normals, 36 * n}, {u->texcoords, 24 * n}, {u->tangents, 36 * n}, {u->material_ids, 4 * n}};
    for (const auto &a : arrays)
        if (int rc = rt::check_device_array(s, a.p, a.bytes, FN_DEVICE); rc != RT_OK)
            return rc;
    return RT_OK;
}
namespace {

// the light half of a PreparedGeometry from the scan's compacted lights (rt::prepare_lights states why the tree is the host path's)
int lights_from_scan(const rt::UpdateScan &scan, uint32_t n, rt::PreparedGeometry &G) {
    const size_t nl = scan.light_prims.size();
    for (size_t k = 0; k < nl; ++k) // ascending and in range, or the arrays were written during the call
        if (scan.light_prims[k] >= n || (k && scan.light_prims[k] <= scan.light_prims[k - 1]))
            return rt::fail(RT_ERR_INVALID_ARG, FN_DEVICE + ": the arrays changed during the call (they must be idle on entry)");
    std::vector<uint32_t> all(nl);
    for (size_t k = 0; k < nl; ++k)
        all[k] = (uint32_t)k;
    // (a scene without lights still has a light tree with a root: build_bvh is root-less only for a scene without triangles)
    rt::prepare_lights(scan.light_pos.data(), n == 0 ? 0u : (uint32_t)std::max<size_t>(nl, 1), all, scan.light_prims.data(), G);
    return RT_OK;
}

// REBUILD where a build reads the arrays on the host (the reference-topology builds; the host collapse of a wide tree): one copy to the
// host, then the host path as it is
int rebuild_staged(rt_scene *s, const rt_geometry_update *u) {
    const size_t n = u->n_triangles;
    std::vector<float> pos(9 * n), nrm(9 * n), uv(6 * n), tan(9 * n);
    std::vector<uint32_t> mat(n);
    if (n) {
        HIP_TRY(hipMemcpyAsync(pos.data(), u->positions, 36 * n, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(nrm.data(), u->normals, 36 * n, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(uv.data(), u->texcoords, 24 * n, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(tan.data(), u->tangents, 36 * n, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(mat.data(), u->material_ids, 4 * n, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    rt_geometry_update h = *u;
    h.positions = pos.data(), h.normals = nrm.data(), h.texcoords = uv.data(), h.tangents = tan.data(), h.material_ids = mat.data();
    return rebuild(s, geometry_desc(s, &h), FN_DEVICE);
}

} // namespace

extern "C" int rt_update_geometry(rt_scene *s, const rt_geometry_update *u) {
    int rc; // before any HIP call
    if ((rc = check_struct(u, FN_HOST, false)) != RT_OK || (rc = check_scene(s, u, FN_HOST)) != RT_OK ||
        (rc = rt::check_geometry_contents(u->material_ids, u->positions, u->n_triangles, s->prep->mats.size(), FN_HOST)) != RT_OK || (rc = check_mode(s, u, FN_HOST)) != RT_OK)
        return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream)); // (every entry point leaves it idle: this costs nothing and says so)
    const rt_scene_desc d = geometry_desc(s, u);
    rc = u->mode == RT_UPDATE_REFIT ? refit(s, u, d) : rebuild(s, d, FN_HOST);
    if (rc == RT_OK) {
        s->pkt = rt::PacketPolicy{};   // measured on the old tree
        s->rebuilt_bvh = rt::HostBvh{}; // reconstructed from the old device tree
    }
    return rc;
}

extern "C" int rt_refit_times(const rt_scene *s, double *refit_ms, double *levels_ms) {
    if (!s || !refit_ms || !levels_ms)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_refit_times: null argument");
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_refit_times: multi-GPU scenes cannot be updated");
    *refit_ms = s->refit_ms;
    *levels_ms = s->refit_levels_ms;
    return RT_OK;
}

extern "C" int rt_update_geometry_device(rt_scene *s, const rt_geometry_update *u) {
    int rc; // before any HIP call
    if ((rc = check_struct(u, FN_DEVICE, true)) != RT_OK || (rc = check_scene(s, u, FN_DEVICE)) != RT_OK)
        return rc;
    HIP_TRY(hipSetDevice(s->device));
    if (u->n_triangles && (rc = rt::check_device_pointers(s, u)) != RT_OK) // before any launch
        return rc;
    return rt::update_from_device_arrays(s, u, false);
}

// Everything rt_update_geometry_device can refuse of device arrays it may read, found without writing anything: the two data-dependent
// refusals, the mode against the scene, the wide tree's exponent range. A shutter accumulator asks this of both keys at attach. `scan`: the
// bounds of the vertices, for the caller.
int rt::refuse_device_arrays(rt_scene *s, const rt_geometry_update *u, const std::string &fn, rt::UpdateScan *scan) {
    const char *what = "";
    const rt::DeviceArrays arrays{u->positions, u->normals, u->texcoords, u->tangents, u->material_ids, u->n_triangles};
    if (hipError_t e = rt::scan_update_device(arrays, rt::emissive_materials(s->prep->mats), false, s->stream, scan, &what); e != hipSuccess)
        return rt::hip_fail(e, fn + ": " + what);
    if (int rc = refuse_scan_findings(*scan, fn); rc != RT_OK)
        return rc;
    if (int rc = check_mode(s, u, fn); rc != RT_OK)
        return rc;
    if (u->n_triangles && s->dev.scene.n_wide != 0u && !rt::wide_grid_in_range(rt::make_wide_grid(scan->lo, scan->hi)))
        return rt::fail(RT_ERR_UNSUPPORTED, fn + ": the new extent is outside the 8-wide tree's exponent range (2^-52 .. 2^52)");
    return RT_OK;
}

// The same scan over positions alone (no material ids: nothing is emissive, no id is checked): the finite-position refusal for arrays that
// are not an update, the keys of rt_accum_attach_flow. Writes nothing but the scan's own scratch.
int rt::refuse_non_finite_positions(rt_scene *s, const float *d_positions, uint32_t n, const std::string &fn) {
    const char *what = "";
    rt::DeviceArrays arrays;
    arrays.pos = d_positions, arrays.n = n;
    rt::UpdateScan scan;
    if (hipError_t e = rt::scan_update_device(arrays, {}, false, s->stream, &scan, &what); e != hipSuccess)
        return rt::hip_fail(e, fn + ": " + what);
    return refuse_scan_findings(scan, fn); // (no ids were scanned: bad_material is unset)
}

// rt_update_geometry_device behind its argument checks: `u` names device arrays of the scene's GPU and of the scene's triangle count, in a
// known mode. Also the path by which a shutter accumulator installs a slice (rt_accum_shutter.cpp), which is why the live-accumulator
// refusal is the entry point's and not this function's. `keep_lights` (REFIT only): the emissive triangles have the positions the live
// light tree was built from, bit for bit, so the light half (a list across the bus, a host build, a tree back) is skipped.
int rt::update_from_device_arrays(rt_scene *s, const rt_geometry_update *u, bool keep_lights) {
    int rc;
    const uint32_t n = u->n_triangles;
    HIP_TRY(hipStreamSynchronize(s->stream));
    const rt::PreparedScene &P = *s->prep;
    const rt::BuildKind kind = rt::build_kind(P.build_flags, n);
    const bool refit = u->mode == RT_UPDATE_REFIT;
    const bool staged = !refit && kind.host_reads; // a rebuild that reads the arrays on the host
    rt::DeviceArrays arrays;
    arrays.pos = u->positions, arrays.nrm = u->normals, arrays.uv = u->texcoords, arrays.tan = u->tangents, arrays.mat = u->material_ids, arrays.n = n;
    // ---- one pass over positions and ids: the two data-dependent refusals, the bounds, the lights (writes only its own scratch)
    rt::UpdateScan scan;
    const char *what = "";
    keep_lights = keep_lights && refit && !staged;
    const bool want_lights = !staged && !keep_lights && check_mode_ok(s, u); // (a call check_mode is about to refuse needs no light list)
    if (hipError_t e = rt::scan_update_device(arrays, rt::emissive_materials(P.mats), want_lights, s->stream, &scan, &what); e != hipSuccess)
        return rt::hip_fail(e, FN_DEVICE + ": " + what);
    if ((rc = refuse_scan_findings(scan, FN_DEVICE)) != RT_OK || (rc = check_mode(s, u, FN_DEVICE)) != RT_OK)
        return rc;
    if (staged)
        rc = rebuild_staged(s, u);
    else if (refit && n == 0)
        rc = RT_OK;
    else {
        std::shared_ptr<rt::PreparedGeometry> G;
        if (!keep_lights) {
            G = std::make_shared<rt::PreparedGeometry>();
            if ((rc = lights_from_scan(scan, n, *G)) != RT_OK)
                return rc;
        }
        if (refit) { // the caller's arrays are the refit's input: nothing is allocated or copied for them, and `in` owns nothing
            rt::RefitInput in;
            in.pos = const_cast<float *>(u->positions), in.nrm = const_cast<float *>(u->normals), in.uv = const_cast<float *>(u->texcoords);
            in.tan = const_cast<float *>(u->tangents), in.mat = const_cast<uint32_t *>(u->material_ids), in.n = n;
            std::memcpy(in.lo, scan.lo, 12);
            std::memcpy(in.hi, scan.hi, 12);
            rc = refit_from(s, G, in, FN_DEVICE);
        } else { // the device build reads them where they are
            rt_geometry_update none = *u; // (no host code may follow these five pointers)
            none.positions = none.normals = none.texcoords = none.tangents = nullptr;
            none.material_ids = nullptr;
            rc = rebuild_from(s, geometry_desc(s, &none), G, &arrays, FN_DEVICE);
        }
    }
    if (rc == RT_OK) {
        s->pkt = rt::PacketPolicy{};
        s->rebuilt_bvh = rt::HostBvh{};
    }
    return rc;
}
