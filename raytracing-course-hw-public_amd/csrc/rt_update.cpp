// rt_update.cpp — rt_update_geometry (include/rt_abi.h): new per-triangle arrays for a built scene, without rt_destroy + rt_create.
//
// Everything that does not follow from the five arrays stays where it is: materials, texture views, the 268 MB texel pool, the tables, the
// analytic primitives, the camera, the stream, the wavefront workspace. What does follow from them is the geometry half of rt_create
// (rt_scene.cpp: prepare_geometry on the host, upload_geometry on the device), and the two modes differ in how much of it runs again:
//   RT_UPDATE_REBUILD  all of it, into new buffers beside the live ones; then swap and free. The scene is the one rt_create would build.
//   RT_UPDATE_REFIT    (RT_BUILD_WIDE) the light half on the host as in REBUILD; the scene tree keeps its topology and is refitted in
//                      place on the device (rt_wide_refit.hip), the triangle and shading records are rewritten in place.
#include <cmath>
#include <cstring>

#include "rt_scene_impl.h"
#include "rt_wide_refit.h"
#include "wide_grid.h"

namespace {

int check_update(const rt_scene *s, const rt_geometry_update *u) {
    if (!u)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_update_geometry: null argument");
    if (u->mode != RT_UPDATE_REBUILD && u->mode != RT_UPDATE_REFIT)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_update_geometry: unknown mode");
    for (uint32_t r : u->reserved)
        if (r)
            return rt::fail(RT_ERR_INVALID_ARG, "rt_update_geometry: reserved field is not 0");
    if (u->n_triangles && (!u->positions || !u->normals || !u->texcoords || !u->tangents || !u->material_ids))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_update_geometry: null geometry array");
    if (!s)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_update_geometry: null scene");
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_update_geometry: multi-GPU scenes cannot be updated");
    if (u->n_triangles != s->dev.n_triangles)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_update_geometry: n_triangles is " + std::to_string(u->n_triangles) + ", the scene has " +
                                                std::to_string(s->dev.n_triangles));
    if (s->live_accums)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_update_geometry: the scene has " + std::to_string(s->live_accums) +
                                                " live accumulator(s), whose sums are of the old geometry: destroy them first");
    const size_t n_mats = s->prep->mats.size();
    for (uint32_t i = 0; i < u->n_triangles; ++i)
        if (u->material_ids[i] >= n_mats)
            return rt::fail(RT_ERR_INVALID_ARG, "rt_update_geometry: material id out of range");
    for (size_t i = 0; i < (size_t)u->n_triangles * 9; ++i) // as rt_create: no builder has an answer for NaN or infinity
        if (!std::isfinite(u->positions[i]))
            return rt::fail(RT_ERR_INVALID_ARG, "rt_update_geometry: non-finite vertex position (triangle " + std::to_string(i / 9) + ")");
    if (u->mode == RT_UPDATE_REFIT && !(s->prep->build_flags & RT_BUILD_WIDE))
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_update_geometry: RT_UPDATE_REFIT needs a scene built with RT_BUILD_WIDE (a refitted binary tree is "
                                            "not the reference's topology): use RT_UPDATE_REBUILD");
    return RT_OK;
}

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

std::vector<uint8_t> emissive_materials(const rt::PreparedScene &P) {
    std::vector<uint8_t> em(P.mats.size());
    for (size_t i = 0; i < em.size(); ++i) {
        const float *e = P.mats[i].emission;
        em[i] = !((e[0] == 0) & (e[1] == 0) & (e[2] == 0));
    }
    return em;
}

void free_list(std::vector<void *> &v) {
    for (void *p : v)
        (void)hipFree(p);
    v.clear();
}

int rebuild(rt_scene *s, const rt_scene_desc &d) {
    const rt::PreparedScene &P = *s->prep;
    auto G = std::make_shared<rt::PreparedGeometry>();
    rt::prepare_geometry(&d, emissive_materials(P), P.wide_cost_node, P.wide_cost_tri, *G);
    // the new buffers are built beside the live ones: a refusal below leaves the scene as it was
    rt::GeometryOnDevice g;
    int rc = rt::upload_geometry(s, &d, P, *G, g);
    hipError_t se = rc == RT_OK ? hipDeviceSynchronize() : hipSuccess; // uploads went through the null stream
    if (rc == RT_OK && se != hipSuccess)
        rc = rt::fail(RT_ERR_HIP, std::string("rt_update_geometry: ") + hipGetErrorString(se));
    if (rc != RT_OK) {
        g.free_all();
        return rc;
    }
    std::vector<void *> old_geo = std::move(s->geo_owned), old_light = std::move(s->light_owned);
    rt::install_geometry(s, g);
    free_list(old_geo);
    free_list(old_light);
    s->geo = G;
    s->refitted = false;
    return RT_OK;
}

int refit(rt_scene *s, const rt_geometry_update *u, const rt_scene_desc &d) {
    const rt::PreparedScene &P = *s->prep;
    DevScene &D = s->dev;
    if (u->n_triangles == 0)
        return RT_OK;
    // ---- host: the light tree and its records, as in REBUILD (the light set follows the new material ids)
    auto G = std::make_shared<rt::PreparedGeometry>();
    rt::prepare_geometry(&d, emissive_materials(P), P.wide_cost_node, P.wide_cost_tri, *G, /*lights_only=*/true);
    // ---- device, part 1: nothing a render kernel reads is written before the update can no longer be refused
    rt::RefitInput in;
    const char *what = "";
    if (hipError_t e = rt::refit_upload(u, s->stream, &in, &what); e != hipSuccess)
        return rt::fail(e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, std::string("rt_update_geometry: ") + what + ": " + hipGetErrorString(e));
    struct FreeInput {
        rt::RefitInput &in;
        ~FreeInput() { in.free_all(); }
    } free_input{in};
    const WideGrid grid = rt::make_wide_grid(in.lo, in.hi);
    if (D.scene.n_wide != 0u && !rt::wide_grid_in_range(grid))
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_update_geometry: the new extent is outside the 8-wide tree's exponent range (2^-52 .. 2^52)");
    rt::GeometryOnDevice lg; // only its light half is filled
    auto upload_lights = [&]() -> int {
        auto up = [&](const void *src, size_t bytes, const void **dst) -> int {
            *dst = nullptr;
            if (!bytes)
                return RT_OK;
            void *p = nullptr;
            HIP_TRY(hipMalloc(&p, bytes));
            lg.light_owned.push_back(p);
            HIP_TRY(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, s->stream));
            *dst = p;
            return RT_OK;
        };
        const rt::FlatBvh &f = G->flat[1];
        int rc;
        if ((rc = up(f.nodes.data(), f.nodes.size() * sizeof(DevNode), (const void **)&lg.lights.nodes)) != RT_OK ||
            (rc = up(f.tris.data(), f.tris.size() * sizeof(DevTri), (const void **)&lg.lights.tris)) != RT_OK ||
            (rc = up(G->laux.data(), G->laux.size() * sizeof(DevLightAux), (const void **)&lg.light_aux)) != RT_OK)
            return rc;
        HIP_TRY(hipStreamSynchronize(s->stream));
        return RT_OK;
    };
    if (int rc = upload_lights(); rc != RT_OK) {
        (void)hipStreamSynchronize(s->stream);
        lg.free_all();
        return rc;
    }
    // ---- device, part 2: records and nodes in place (its scratch is allocated first: RT_ERR_OOM still leaves the scene as it was)
    if (hipError_t e = rt::refit_wide_device(in, const_cast<DevTri *>(D.scene.tris), const_cast<DevAttr *>(D.attrs), D.scene.n_tris, const_cast<uint4_pod *>(D.scene.wide),
                                             D.scene.n_units, D.scene.n_wide, grid, s->stream, &what);
        e != hipSuccess) {
        (void)hipStreamSynchronize(s->stream);
        lg.free_all();
        return rt::fail(e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, std::string("rt_update_geometry: ") + what + ": " + hipGetErrorString(e));
    }
    // ---- host: what the launches read of the tree besides the blob
    const rt::FlatBvh &f = G->flat[1];
    DevBvh &L = D.lights;
    const DevNode *ln = lg.lights.nodes;
    const DevTri *lt = lg.lights.tris;
    L = DevBvh{};
    L.nodes = ln;
    L.tris = lt;
    L.root = f.root;
    L.n_tris = (uint32_t)f.tris.size();
    L.fast_ok = f.fast_ok ? 1u : 0u;
    L.lds_inner = rt::light_lds_inner(f);
    D.light_aux = lg.light_aux;
    s->dev_n_inner[1] = (uint32_t)f.nodes.size();
    free_list(s->light_owned);
    s->light_owned = std::move(lg.light_owned);
    D.scene.grid = grid;
    for (int k = 0; k < 3; ++k)
        rt::sort_bounds_axis(in.lo[k], in.hi[k], D.bounds_lo[k], D.bounds_inv[k]);
    s->geo = G; // (its host_bvh[0] / wide are empty: the tree the wide one was collapsed from no longer describes the scene)
    s->refitted = true;
    return RT_OK;
}

} // namespace

extern "C" int rt_update_geometry(rt_scene *s, const rt_geometry_update *u) {
    if (int rc = check_update(s, u); rc != RT_OK) // before any HIP call
        return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream)); // (every entry point leaves it idle: this costs nothing and says so)
    const rt_scene_desc d = geometry_desc(s, u);
    const int rc = u->mode == RT_UPDATE_REFIT ? refit(s, u, d) : rebuild(s, d);
    if (rc == RT_OK) {
        s->pkt = rt::PacketPolicy{};   // measured on the old tree
        s->rebuilt_bvh = rt::HostBvh{}; // reconstructed from the old device tree
    }
    return rc;
}
