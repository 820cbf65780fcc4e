// rt_scene_impl.h — what the host files behind include/rt_abi.h share (internal): the definition of rt_scene and the few helpers
// with more than one user. rt_scene_prepare.cpp is the host half of rt_create, rt_scene.cpp its device half with the entry points that create and destroy scenes; rt_render.cpp (rt_render*), rt_rays.cpp (rt_render_rays*), rt_bake.cpp (rt_bake*, rt_lightmap_points),
// rt_accum_host.cpp and rt_accum_layers.cpp (rt_accum_*, over rt_accum_impl.h) and rt_probe.cpp (probes, BVH dumps) run on them. rt_group.cpp sees rt_scene as an opaque type through
// rt_group.h. The arrays of a call, on the host or in the caller's HBM, are declared on an rt::CallIo (rt_call_io.h) over the scene's one
// staging block; its run() and timed_call below are the brackets every entry point queues its work in.
#pragma once
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rt_abi.h"
#include "bvh_build.h"
#include "rt_bvh_device.h"
#include "rt_call_io.h"
#include "rt_dev_mem.h"
#include "rt_device_types.h"
#include "rt_error.h"
#include "rt_film.h"
#include "rt_group.h"
#include "rt_kernels.h"
#include "wide_build.h"

namespace rt {
// wf_extend_packet (primary rays as coherent packets) pays off only while a wave's 64 rays stay together; its own census
// (lanes served per trip) decides per configuration whether later passes keep using it. One per owner of passes: the scene for
// rt_render*, every accumulator for its own (rt_render.cpp launch_pass).
struct PacketPolicy {
    uint64_t key = 0; // the configuration `off` was measured on
    bool off = false;
    uint32_t lanes_x100 = 0; // last packet census: lanes served per trip x 100 (rt_stats.packet_lanes_x100)
};

// How a scene of n triangles created with build_flags gets its scene tree: the one derivation for rt_create and both update entry points.
struct BuildKind {
    bool dev_build, wide_build; // rt_bvh_device.hip builds the binary tree / the tree in HBM is the 8-wide one
    bool device_collapse;       // ... emitted on the device too (scenes of a handful of triangles and RT_BUILD_WIDE_HOST_COLLAPSE collapse on the host)
    bool host_reads;            // some step reads the five arrays on the host: the reference-topology builds, the host collapse
};
inline BuildKind build_kind(uint32_t build_flags, uint32_t n) {
    const bool dev = n > 0 && (build_flags & RT_BUILD_DEVICE_LBVH), wide = n > 0 && (build_flags & RT_BUILD_WIDE);
    const bool emitted = dev && wide && !(build_flags & RT_BUILD_WIDE_HOST_COLLAPSE) && n > 8u;
    return {dev, wide, emitted, !dev || (wide && !emitted)};
}
// What the queries report of a build (rt_build_times*, rt_wide_info, the BVH dumps) and the launch policy reads.
struct BuildFacts {
    bool device_built = false; // scene BVH built by rt_bvh_device.hip
    bool wide_built = false;   // RT_BUILD_WIDE: the 8-wide quantised tree (wide_build.cpp); host_bvh[0] is the binary tree it was collapsed from when built on the host
    uint32_t wide_depth = 0;
    double wide_ms = 0, wide_cost = 0, build_ms = 0, build_upload_ms = 0;
    uint32_t dev_n_inner[2] = {0, 0}; // inner nodes of the binary trees in HBM: scene (0 for a wide one), lights
};

// The host half of rt_create comes in two halves. The GEOMETRY half is everything that follows from the five per-triangle arrays: both
// trees, the triangle, shading and light records. rt_update_geometry makes a new one; the other half (below) is never copied for that.
struct PreparedGeometry {
    HostBvh host_bvh[2];
    FlatBvh flat[2];            // [0] empty when the scene BVH is built on the device or is wide
    WideBvh wide;               // BuildKind: wide_build && !dev_build
    std::vector<DevTri> wide_tris;
    std::vector<DevAttr> attrs; // scene-BVH order (empty when built on the device)
    std::vector<DevLightAux> laux;
    double build_ms = 0, wide_ms = 0;
};
// ... and the rest: materials, texture views, the texel pool, tables, and how the scene asked to be built. Shared by the replicas of a
// multi-GPU scene; a scene keeps it for life.
struct PreparedScene {
    std::shared_ptr<const PreparedGeometry> geo; // of the creation arrays
    std::vector<DevMaterial> mats;
    std::vector<DevTexture> texs;
    std::vector<uint32_t> pool;
    std::vector<rt_primitive_desc> prims;
    std::vector<float> lut_lin, lut_gam;
    int32_t bg_view = -1;       // view of rt_scene_desc.bg_texture in texs (stand-alone), -1 = the white default
    float wide_cost_node = 1.0f, wide_cost_tri = 0.3f;
    uint32_t build_flags = 0;   // rt_scene_desc.build_flags / .build as created: what rt_update_geometry rebuilds with
    rt_build_options build{};
};

// What the geometry half leaves on one device (rt_scene.cpp upload_geometry): the buffers it allocated, the two trees as the kernels
// address them, and the build facts. The buffers die with the struct unless install_geometry hands them to the scene.
struct GeometryOnDevice {
    DevArena owned;       // scene tree, triangle records, shading records
    DevArena light_owned; // light tree, its triangle records, DevLightAux
    DevBvh scene{}, lights{};
    const DevAttr *attrs = nullptr;
    const DevLightAux *light_aux = nullptr;
    float bounds_lo[3] = {0, 0, 0}, bounds_inv[3] = {0, 0, 0};
    BuildFacts facts;
};

// The wide kernels' exponent arithmetic stays among normal floats while the scene's largest cell exponent (e_base + 15) lies in [-60, 44]
// (rt_scene.cpp pack_wide_tree states why): the one test rt_create and rt_update_geometry make on a grid.
inline bool wide_grid_in_range(const WideGrid &grid) { return !(grid.e_base + 15 < -60 || grid.e_base + 15 > 44); }
// one axis of the ray-ordering key's scene box: lower bound and 1 / extent (0 for a flat axis)
inline void sort_bounds_axis(float lo, float hi, float &bounds_lo, float &bounds_inv) {
    bounds_lo = lo;
    bounds_inv = (hi > lo) ? 1.0f / (hi - lo) : 0.0f;
}
} // namespace rt

struct rt_scene {
    rt::Group *group = nullptr; // multi-GPU scene: replicas + RCCL communicator (rt_group.cpp); the fields below stay unused
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    rt::EventPool ext_events; // (start, stop) per wf_extend launch of the current render; reused by every render
    DevScene dev{};
    rt_camera cam{};
    rt::DevArena owned;       // what lives as long as the scene: materials, textures, texels, tables, counters
    rt::DevArena geo_owned;   // the scene tree and its records ...
    rt::DevArena light_owned; // ... and the light tree's: freed when rt_update_geometry swaps new ones in
    rt::DevArena env_owned;   // the float environment of rt_set_environment (DevScene::env): texels and tables; empty without one
    std::shared_ptr<const rt::PreparedScene> prep; // the host half of rt_create, shared by the replicas of a multi-GPU scene
    std::shared_ptr<const rt::PreparedGeometry> geo; // its geometry half: prep->geo until rt_update_geometry replaces it
    uint32_t live_accums = 0;  // accumulators of this scene (rt_accum_create* / rt_accum_destroy): their sums pin the geometry
    uint32_t shutter_accums = 0; // ... of which have a shutter (rt_accum_attach_shutter): it moves the geometry, so it must be the only one
    bool refitted = false;     // the wide tree was refitted: the binary tree it was collapsed from no longer describes the scene
    rt::HostBvh rebuilt_bvh;   // device-built scene BVH: the reference-style node list, reconstructed from HBM on demand
    rt::BuildFacts facts;      // of the trees in HBM (install_geometry; a refit renews dev_n_inner[1])
    double refit_ms = 0, refit_levels_ms = 0; // the last RT_UPDATE_REFIT: refit_wide_device in all, and its top-down level pass (rt_refit_times)
    uint32_t *d_counter = nullptr; // both of `owned`
    DevStats *d_stats = nullptr;
    uint64_t second_visits = 0;    // DevStats::second_visits of the last call that counted (rt_second_visits)
    // Buffers grown on demand (rt::DevBuf: the content does not survive growth, a failed growth leaves them empty):
    rt::DevBuf<uint8_t> staging;      // what a call stages of its arrays: host inputs, host or internal outputs (rt_call_io.h), in bytes
    rt::DevBuf<rt::FilmTable> film_table; // the verified threshold table (host/film.cpp), uploaded by the first ensure_film
    rt::DevBuf<WfSensor> sensors;     // the camera table of a render's wavefront passes (WfLaunch::sensors: one record per view or sensor) / the one
                                      // record of rt_sensor_rays

    // device film prerequisite: the threshold table
    int ensure_film() {
        if (!film_table.get()) {
            rt::FilmTable t{};
            if (!rt::film_table(t.thr, t.special))
                return rt::fail(RT_ERR_UNSUPPORTED, "device film: the host libm's powf failed the monotonicity check; use rt_render + rt_tonemap_rgb8");
            HIP_TRY(film_table.reserve(1));
            HIP_TRY(hipMemcpyAsync(film_table.get(), &t, sizeof(t), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipStreamSynchronize(stream)); // `t` is a local
        }
        return RT_OK;
    }
    int ensure_sensors(uint32_t n) {
        HIP_TRY(sensors.reserve(n));
        return RT_OK;
    }
    int num_cus = 0;
    int blocks_per_cu = 8; // upper bound on resident 256-thread blocks per CU; surplus blocks find the ticket exhausted
    // wavefront pipeline workspace (rt_wavefront.hip), sized for wf_paths_cap paths / wf_pixels_cap pixels per pass
    uint64_t wf_paths_cap = 0, wf_pixels_cap = 0;
    uint32_t wf_depth_cap = 0;
    rt::DevArena wf_owned{16};
    WfPath *wf_paths[2] = {nullptr, nullptr};
    uint32_t *wf_stripes = nullptr;
    WfHit *wf_hits = nullptr;
    WfFold *wf_fold = nullptr;
    RtF4 *wf_samples = nullptr, *wf_accum = nullptr;
    uint32_t *wf_counters = nullptr;
    void *wf_stack_overflow = nullptr; // wf_extend's evicted stack frames (RingStackT): RT_MAX_STACK x grid threads x 16 B
    uint32_t wf_stack_stride = 0;
    uint32_t *wf_sort_keys[2] = {nullptr, nullptr}, *wf_sort_vals[2] = {nullptr, nullptr};
    void *wf_sort_temp = nullptr;
    size_t wf_sort_temp_bytes = 0;
    uint32_t *wf_host_count = nullptr; // pinned, 48 words: queue size per bounce, then wf_extend_packet's census (rt_kernels.h WfHostSync)
    std::vector<hipEvent_t> wf_count_events; // one per bounce: "the size of the queue entering this bounce has reached wf_host_count"
    rt::PacketPolicy pkt; // of rt_render* (an accumulator keeps its own)
    rt::PacketPolicy pkt_sensor[6]; // of rt_render_sensors*: one per kind for a single sensor, [5] for several: a panorama's census never switches rt_render's packets off
    std::vector<hipEvent_t> pass_events; // rt_params.progress: one per pass

    // The camera-relative copy of the binary scene tree's records (WfLaunch::rel_nodes / rel_tris): part of the wavefront workspace, made by
    // launch_pass for the passes whose primary rays share one origin and kept while (camera position, tree) stay the same. `rel_gen` is the
    // geo_generation the copy was made of; every swap or in-place rewrite of the tree (install_geometry, a refit) moves geo_generation on.
    rt::DevBuf<uint8_t> wf_rel;    // the one allocation behind both: node records first, then triangle records (bytes)
    DevTri *wf_rel_tris = nullptr; // where the triangle records of the current copy begin
    uint64_t geo_generation = 1, wf_rel_gen = 0; // 0: no valid copy
    uint32_t wf_rel_pos[3] = {0, 0, 0}; // the camera position of the copy, as bits

    int ensure_wavefront(uint64_t paths, uint64_t pixels, uint32_t depth) {
        if (paths <= wf_paths_cap && pixels <= wf_pixels_cap && depth <= wf_depth_cap)
            return RT_OK;
        wf_owned.reset();
        wf_paths_cap = wf_pixels_cap = 0;
        wf_depth_cap = 0;
        auto alloc = [&](size_t bytes, void **out) -> int {
            if (hipError_t e = wf_owned.alloc_bytes(out, bytes); e != hipSuccess)
                return rt::hip_fail(e, "wavefront workspace");
            return RT_OK;
        };
        int rc;
        // + 64: wf_shade's sub-queue regions cover whole wave slots (rt_device_types.h, WF_STRIPES)
        if ((rc = alloc((paths + 64) * sizeof(WfPath), (void **)&wf_paths[0])) != RT_OK || (rc = alloc((paths + 64) * sizeof(WfPath), (void **)&wf_paths[1])) != RT_OK ||
            (rc = alloc(WF_STRIPE_BUF_WORDS * sizeof(uint32_t), (void **)&wf_stripes)) != RT_OK ||
            (rc = alloc(paths * sizeof(WfHit), (void **)&wf_hits)) != RT_OK || (rc = alloc(paths * depth * 2 * sizeof(WfFold), (void **)&wf_fold)) != RT_OK ||
            (rc = alloc(paths * sizeof(RtF4), (void **)&wf_samples)) != RT_OK || (rc = alloc(pixels * sizeof(RtF4), (void **)&wf_accum)) != RT_OK ||
            (rc = alloc(WF_CNT_ALLOC_WORDS * sizeof(uint32_t), (void **)&wf_counters)) != RT_OK)
            return rc;
        wf_stack_stride = (uint32_t)num_cus * 8u * 256u; // the wf_extend grid: 8 blocks of 256 threads per CU
        if ((rc = alloc((size_t)RT_MAX_STACK * wf_stack_stride * 16, &wf_stack_overflow)) != RT_OK)
            return rc;
        // + 64: the ray-order sort runs over the queue's physical positions, whole wave slots like the queues above
        wf_sort_temp_bytes = rt::wavefront_sort_temp_bytes(paths + 64);
        if ((rc = alloc((paths + 64) * 4, (void **)&wf_sort_keys[0])) != RT_OK || (rc = alloc((paths + 64) * 4, (void **)&wf_sort_keys[1])) != RT_OK ||
            (rc = alloc((paths + 64) * 4, (void **)&wf_sort_vals[0])) != RT_OK || (rc = alloc((paths + 64) * 4, (void **)&wf_sort_vals[1])) != RT_OK ||
            (rc = alloc(wf_sort_temp_bytes, &wf_sort_temp)) != RT_OK)
            return rc;
        // on the scene's own (non-blocking) stream: a null-stream memset is not ordered with the kernels launched there and
        // could land after the first stage had set the queue size
        HIP_TRY(hipMemsetAsync(wf_counters, 0, WF_CNT_ALLOC_WORDS * sizeof(uint32_t), stream));
        wf_paths_cap = paths;
        wf_pixels_cap = pixels;
        wf_depth_cap = depth;
        return RT_OK;
    }

    // The per-path records of an accumulator's layers (null: it keeps none), sized like the wavefront workspace and allocated the first time
    // such an accumulator renders on this scene: two feature records per path (WfFeat::rec, 32 B), one id (WfIds::rec, 4 B), n_groups group
    // records (WfGroups::rec, 16 B each), one tag byte per path and frame level (WfGroups::tag) and one flow record (WfFlow::rec, 16 B). None
    // needs its content kept or cleared (a stale tag is legal: WfGroups). Call after ensure_wavefront.
    rt::DevBuf<RtF4> wf_feat;
    rt::DevBuf<uint32_t> wf_ids;
    rt::DevBuf<RtF4> wf_group_rec;
    rt::DevBuf<uint8_t> wf_group_tag;
    rt::DevBuf<RtF4> wf_flow;
    int bind_layer_records(WfFeat *features, WfIds *ids, WfGroups *groups, WfFlow *flow) {
        auto reserve = [](auto &buf, size_t count, const char *what) -> int {
            if (hipError_t e = buf.reserve(count); e != hipSuccess)
                return rt::hip_fail(e, what);
            return RT_OK;
        };
        if (int rc = features ? reserve(wf_feat, wf_paths_cap * 2, "feature records") : RT_OK; rc != RT_OK)
            return rc;
        if (int rc = ids ? reserve(wf_ids, wf_paths_cap, "id records") : RT_OK; rc != RT_OK)
            return rc;
        if (int rc = groups ? reserve(wf_group_rec, wf_paths_cap * groups->n_groups, "light-group records") : RT_OK; rc != RT_OK)
            return rc;
        if (int rc = groups ? reserve(wf_group_tag, wf_paths_cap * (wf_depth_cap + 1ull), "light-group tags") : RT_OK; rc != RT_OK)
            return rc;
        if (int rc = flow ? reserve(wf_flow, wf_paths_cap, "flow records") : RT_OK; rc != RT_OK)
            return rc;
        if (flow)
            flow->rec = wf_flow.get();
        if (features)
            features->rec = wf_feat.get();
        if (ids)
            ids->rec = wf_ids.get();
        if (groups)
            groups->rec = wf_group_rec.get(), groups->tag = wf_group_tag.get();
        return RT_OK;
    }
    // the workspace half of a WfLaunch (after ensure_wavefront): queues, hit records, counters, stack workspace, sort buffers
    void wf_bind(WfLaunch &W) {
        W.paths_in = wf_paths[0];
        W.paths_out = wf_paths[1];
        W.hits = wf_hits;
        W.fold = wf_fold;
        W.sample_out = wf_samples;
        W.accum = wf_accum;
        W.counters = wf_counters;
        W.stripes = wf_stripes;
        W.stack_overflow = wf_stack_overflow;
        W.stack_stride = wf_stack_stride;
        for (int k = 0; k < 2; ++k) { // sort_vals[1] also carries the unsorted order (sort_mode 0)
            W.sort_keys[k] = wf_sort_keys[k];
            W.sort_vals[k] = wf_sort_vals[k];
        }
        W.sort_temp = wf_sort_temp;
        W.sort_temp_bytes = wf_sort_temp_bytes;
        W.packet_census = reinterpret_cast<unsigned long long *>(wf_counters + WF_CNT_CENSUS);
    }

    ~rt_scene() {
        if (group) {
            rt::group_destroy(group);
            return;
        }
        (void)hipSetDevice(device);
        if (wf_host_count)
            (void)hipHostFree(wf_host_count);
        for (hipEvent_t ev : wf_count_events)
            (void)hipEventDestroy(ev);
        for (hipEvent_t ev : pass_events)
            (void)hipEventDestroy(ev);
        // Device memory goes before the stream it was used on, as it always has: the members' own destructors run after this body, that is
        // after hipStreamDestroy (an owner not named here is still freed then, with `device` current). Nothing is in flight: every entry
        // point returns with the stream synchronised. In a group's handle all of them are empty.
        for (rt::DevArena *a : {&wf_owned, &owned, &geo_owned, &light_owned, &env_owned})
            a->reset();
        wf_feat.reset(), wf_ids.reset(), wf_group_rec.reset(), wf_group_tag.reset(), wf_flow.reset(), wf_rel.reset(), staging.reset(), sensors.reset(), film_table.reset();
        ext_events.destroy();
        if (ev0)
            (void)hipEventDestroy(ev0);
        if (ev1)
            (void)hipEventDestroy(ev1);
        if (stream)
            (void)hipStreamDestroy(stream);
    }
};

namespace rt {
// the two refusals for the contents of geometry arrays, whoever found the fault: a host loop (check_geometry_contents) or the device scan
inline int refuse_material(const std::string &fn) { return fail(RT_ERR_INVALID_ARG, fn + ": material id out of range"); }
inline int refuse_non_finite(const std::string &fn, size_t triangle) {
    return fail(RT_ERR_INVALID_ARG, fn + ": non-finite vertex position (triangle " + std::to_string(triangle) + ")");
}
// rt_scene_prepare.cpp: the host half of the geometry build, which rt_create and rt_update_geometry (rt_update.cpp) both run, and its steps
// with a second user: the refusals for the arrays' contents (`fn` names the entry point) and the records of a wide tree collapsed on the host
int check_geometry_contents(const uint32_t *material_ids, const float *positions, uint32_t n, size_t n_materials, const std::string &fn);
void prepare_geometry(const rt_scene_desc *d, const std::vector<uint8_t> &emissive, float wide_cost_node, float wide_cost_tri, PreparedGeometry &P,
                      bool lights_only = false);
std::vector<uint8_t> emissive_materials(const std::vector<DevMaterial> &mats); // one byte per material: does it emit?
void prepare_lights(const float *positions, uint32_t n_total, const std::vector<uint32_t> &lights, const uint32_t *original, PreparedGeometry &P);
void make_attrs(const rt_scene_desc *d, const std::vector<DevTri> &tris, std::vector<DevAttr> &attrs);
void make_wide_tris(const rt_scene_desc *d, const WideBvh &wide, std::vector<DevTri> &tris);
// rt_scene.cpp: the device half
const HostBvh &prepared_host_bvh(const rt_scene *s, int which); // the host-built trees kept by the scene's PreparedGeometry
int upload_geometry(rt_scene *s, const rt_scene_desc *d, const PreparedScene &PS, const PreparedGeometry &P, GeometryOnDevice &out,
                    const DeviceArrays *arrays = nullptr);
int upload_light_tree(const FlatBvh &f, const std::vector<DevLightAux> &laux, DevArena &owned, hipStream_t stream, DevBvh &tree, const DevLightAux *&aux, uint32_t &n_inner);
void install_geometry(rt_scene *s, GeometryOnDevice &g);
// rt_update.cpp: the update from device arrays behind rt_update_geometry_device's argument checks, and those of its checks a shutter
// accumulator (rt_accum_shutter.cpp) makes of its keys at attach
struct UpdateScan;
int check_device_pointers(const rt_scene *s, const rt_geometry_update *u);
int check_device_array(const rt_scene *s, const void *p, size_t bytes, const std::string &fn); // one array of them, named by the caller's `fn`
int refuse_device_arrays(rt_scene *s, const rt_geometry_update *u, const std::string &fn, UpdateScan *scan);
int refuse_non_finite_positions(rt_scene *s, const float *d_positions, uint32_t n, const std::string &fn);
int update_from_device_arrays(rt_scene *s, const rt_geometry_update *u, bool keep_lights);
// rt_render.cpp: the checks of rt_params, the wavefront pass policy, the pass loop and the statistics of a finished call
void set_camera(DevScene &D, const float *pos, const float *right, const float *up, const float *fwd);
int check_pass_params(const rt_params *p, const char *fn);
int check_wavefront_entry(const rt_params *p, const char *fn, const char *subject, uint32_t flags_taken, bool reads_samples);
uint64_t wavefront_max_paths(rt_scene *s, const rt_params *p);
WfLaunch one_row_launch(const rt_scene *s, const rt_params *p, uint32_t n, uint32_t samples, float *fb, bool counters);
hipError_t launch_pass(rt_scene *s, const rt_params *p, PacketPolicy &pol, WfLaunch &W, const WfPassKind &kind, const WfPassStep &step);
int run_passes(rt_scene *s, const rt_params *p, PacketPolicy &pol, WfLaunch &W, const WfPassKind &kind, uint64_t n_pixels, uint32_t samples, rt_stats *stats,
               const char *fn);
// the image of a single-GPU scene through the cameras of `table` (views as pinhole records, or the checked records of rt_sensor.cpp)
int render_image(rt_scene *s, const rt_params *p, const std::vector<WfSensor> &table, PacketPolicy &pol, float *fb_rgb, uint8_t *rgb8_out, rt_stats *stats);
// rt_sensor.cpp: the argument checks of one rt_sensor, the device record of a sensor or of a view {camera, seed} (single_origin: rt_kernels.h)
int check_sensor(const rt_sensor &sn, uint32_t width, uint32_t height, const char *fn);
WfSensor make_sensor(const rt_sensor &sn, uint32_t width, uint32_t height);
WfSensor make_sensor(const rt_camera &cam, uint64_t seed, uint32_t width, uint32_t height);
void traversal_stats(const DevStats &h, rt_stats *stats); // the counters of the walks, scene and light tree, as rt_stats names them
int fill_stats(rt_scene *s, bool counters, uint64_t samples, std::chrono::steady_clock::time_point wall0, uint32_t packet_lanes_x100, rt_stats *stats);

// The bracket of a call that runs wavefront passes and reports rt_stats (queue_and_wait, rt_call_io.h): the device counters start from zero
// (`counters`), the staged inputs of `io` (null: the call stages nothing) go up, then ev0, `body` (the passes and what belongs to their
// time), ev1, the copies back to the host, and the wait: the kernel time counts neither copy. fill_stats reads the events and the counters
// afterwards.
template <class Body> int timed_call(rt_scene *s, bool counters, CallIo *io, Body body) {
    s->ext_events.reset();
    if (int rc = io ? io->reserve() : RT_OK; rc != RT_OK) // (nothing to do where the caller needed its pointers earlier)
        return rc;
    return queue_and_wait(s->stream, [&]() -> int {
        if (counters)
            HIP_TRY(hipMemsetAsync(s->d_stats, 0, sizeof(DevStats), s->stream));
        if (int rc = io ? io->upload() : RT_OK; rc != RT_OK)
            return rc;
        HIP_TRY(hipEventRecord(s->ev0, s->stream));
        if (int rc = body(); rc != RT_OK)
            return rc;
        HIP_TRY(hipEventRecord(s->ev1, s->stream));
        return io ? io->download() : RT_OK;
    });
}
} // namespace rt
