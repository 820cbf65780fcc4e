// rt_kernels.h — launchers of the HIP kernels (internal; the public boundary is include/rt_abi.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <type_traits>
#include <variant>
#include <vector>

#include "rt_device_types.h"

// Launch + check. hipGetLastError() reports the last error of ANY earlier HIP call of this thread (e.g. a refused
// hipSetDevice in another scene's rt_create), so the sticky state is cleared first: what comes back belongs to this launch.
#define RT_LAUNCH_CHECKED(...)               \
    ({                                       \
        (void)hipGetLastError();             \
        hipLaunchKernelGGL(__VA_ARGS__);     \
        hipGetLastError();                   \
    })
// ... inside a launcher that returns hipError_t: a failed launch (bad configuration, lost device) ends it with that error, so it cannot turn
// into a silently wrong image
#define WF_LAUNCH(...)                                  \
    do {                                                \
        if (hipError_t le_ = RT_LAUNCH_CHECKED(__VA_ARGS__); le_ != hipSuccess) \
            return le_;                                 \
    } while (0)

// Run-time bools -> template arguments: with_bools(f, a, b) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}); inside f the
// arguments are constant expressions (`kernel<A, B>`, `if constexpr (A)`). Every launcher picks its kernel instantiation this way.
template <class F> auto with_bools(F &&f) { return f(); }
template <class F, class... Rest> auto with_bools(F &&f, bool b, Rest... rest) {
    return b ? with_bools([&](auto... c) { return f(std::true_type{}, c...); }, rest...) : with_bools([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

namespace rt {
// HIP events for per-launch timing, created once per scene and reused by every render (no create/destroy inside the
// timed region). next() returns nullptr when an event cannot be created; pairs are taken in (start, stop) order.
struct EventPool {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    hipEvent_t next() {
        if (used == ev.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess)
                return nullptr;
            ev.push_back(e);
        }
        return ev[used++];
    }
    void reset() { used = 0; }
    void destroy() {
        for (hipEvent_t e : ev)
            (void)hipEventDestroy(e);
        ev.clear();
        used = 0;
    }
};
// rt_kernels.hip: persistent megakernel (reference-RNG parity mode; cross-check of the wavefront path) + probes
hipError_t launch_render(const DevScene &S, const RenderLaunch &L, bool stats, int blocks, hipStream_t stream);
hipError_t launch_cast(const DevScene &S, const float *rays, uint32_t n, uint32_t *prim, float *bct, hipStream_t stream);
hipError_t launch_surface_normals(const DevScene &S, const float *rays, uint32_t n, uint32_t *prim, float *t, float *normal, float *shading, hipStream_t stream);
hipError_t launch_light_pdf(const DevScene &S, const float *rays, uint32_t n, float *pdf, hipStream_t stream);
hipError_t launch_bg_at(const DevScene &S, const float *dirs, uint32_t n, float *rgb, hipStream_t stream);
// rt_wavefront.hip: one pass (pixel tile x sample range) of the wavefront pipeline, stream-ordered. It schedules the stages; the closest-hit
// kernels are rt_wf_extend.hip's and rt_wide.hip's, wf_shade is rt_wf_shade.hip's (their launchers: below)
// `extend_events`: with WfPassStep::time_extends, one (start, stop) event pair per wf_extend launch is taken from the pool and recorded on `stream`
// `packet_census_out` (optional, host, 2 words): trips and lanes served of this pass's wf_extend_packet launch (0, 0 if it did not run)
// `host_sync` (optional): pinned words + events for the one-bounce-late read-back of the queue sizes (coherence sort and the
// early stop need an upper bound of the queue on the host); without it bounces >= 1 run unsorted over the full pass
struct WfHostSync {
    uint32_t *counts;    // pinned host memory: word b = size of the queue entering bounce b; words WF_HOST_CENSUS_WORD.. = packet census
    hipEvent_t *events;  // events[b] is recorded once counts[b] has been written
    int n_events;
};
#define WF_HOST_CENSUS_WORD 40 /* 8-byte aligned, behind RT_MAX_RAY_DEPTH + 1 size words */
// The kind of a wavefront pass: where a path's first ray comes from and where its finished samples go. Every pass runs the same pipeline
// (first stage, ray_depth x (extend, shade, advance), wf_fold, last stage); the kind names the first stage's source, the launches that
// follow bounce 0's closest hits and the last stage, and carries exactly what those read. Made by one of the four named constructors only:
//   cameras  the camera table WfLaunch::sensors (a view is a pinhole record), whatever the entry point; wf_resolve adds onto the image
//   list     an accumulator round's entry list; wf_resolve_list adds onto the accumulator's sums, behind the feature sums and the id tables
//            of an accumulator that keeps them (wf_features / wf_ids after bounce 0, wf_resolve_features / wf_resolve_ids before the sums),
//            and behind the group sums of one with light groups (wf_group_tags at every bounce, wf_fold_groups, wf_resolve_groups) and the
//            motion vectors of one with flow (wf_flow after bounce 0, wf_resolve_flow)
//   rays     the caller's rays and streams (rt_render_rays); wf_resolve adds onto the outputs
//   bake     the samples of bake points (rt_bake); wf_resolve_bake folds them as the bake's kind asks
// A camera source is made of the call's camera table on the host (run_passes uploads it as WfLaunch::sensors), a list of its accumulator's one
// camera record; both keep rt::single_origin of it (rt_sensor.cpp): the three floats every ray of the pass starts at, or null.
const float *single_origin(const WfSensor *table, uint32_t n);
// What a list pass keeps besides the sums (host only; all null: nothing): an accumulator's optional layers. wf_features and wf_ids run behind
// bounce 0's closest hits, whose results are final there, and so does wf_flow; wf_group_tags at every bounce, wf_fold_groups before wf_fold;
// then wf_resolve_features, wf_resolve_ids, wf_resolve_groups and wf_resolve_flow, in that order, before wf_resolve_list.
struct WfLayers {
    const WfFeat *features;
    const WfIds *ids;
    const WfGroups *groups;
    const WfFlow *flow;
};
class WfPassKind {
public:
    enum Source { CAMERAS, LIST, RAYS, BAKE };
    static WfPassKind cameras(const WfSensor *table, uint32_t n_views) { return WfPassKind(Cameras{table, n_views, single_origin(table, n_views)}); }
    static WfPassKind list(const WfAccum &entries, const WfLayers &layers, const WfSensor &camera) { return WfPassKind(List{entries, layers, single_origin(&camera, 1)}); }
    static WfPassKind rays(const WfRays &rays) { return WfPassKind(rays); }
    static WfPassKind bake(const WfBake &bake) { return WfPassKind(bake); }

    Source source() const { return (Source)v.index(); }
    // what the source's first and last stages read (the source is the caller's to ask for: std::get throws on another)
    const WfAccum &entries() const { return std::get<List>(v).entries; }
    const WfRays &ray_buffer() const { return std::get<WfRays>(v); }
    const WfBake &bake_points() const { return std::get<WfBake>(v); }
    WfLayers layers() const { return source() == LIST ? std::get<List>(v).layers : WfLayers{}; } // of a list; every other source keeps none
    // the cameras of the pass: part of the packet policy's key (a caller's rays and bake points count as one)
    uint32_t n_views() const { return source() == CAMERAS ? std::get<Cameras>(v).n_views : 1u; }
    const WfSensor *camera_table() const { return source() == CAMERAS ? std::get<Cameras>(v).table : nullptr; } // [n_views], host; null: no table to upload
    // Camera-relative records are for the one view of a camera source (a list has one camera) whose rays share an origin: that origin, else null
    const float *relative_origin() const { return source() == CAMERAS ? std::get<Cameras>(v).origin : source() == LIST ? std::get<List>(v).origin : nullptr; }
    // RT_PACKET_AUTO never picks packets for a bake: a point's samples share an origin and nothing else (a hemisphere or the whole sphere of
    // directions is no packet); RT_PACKET_ON still does, and changes no bit
    bool auto_packets() const { return source() != BAKE; }

private:
    struct Cameras {
        const WfSensor *table;
        uint32_t n_views;
        const float *origin;
    };
    struct List {
        WfAccum entries;
        WfLayers layers;
        const float *origin;
    };
    std::variant<Cameras, List, WfRays, WfBake> v; // in the order of Source
    template <class T> explicit WfPassKind(const T &t) : v(t) {}
};
// This pass of its call: the first / last sample pass of its pixel tile (wf_resolve and wf_resolve_bake start from zero / divide and write
// out; a list's passes are each both), and whether the extend launches are timed (rt_stats::dominant_ms).
struct WfPassStep {
    bool first_pass, last_pass, time_extends;
};
hipError_t launch_wavefront_pass(const DevScene &S, WfLaunch L, const WfPassKind &kind, const WfPassStep &step, bool stats, int num_cus, hipStream_t stream,
                                 EventPool *extend_events, unsigned long long *packet_census_out, const WfHostSync *host_sync);
// rt_bake_rays: the n = points x samples rt_ray records of samples [B.first_sample, B.first_sample + samples) of the points of `B` (device;
// B.out is not read) -> `d_rays_out` (device, 32 B per record, 16-byte aligned)
hipError_t launch_bake_rays(const WfBake &B, uint32_t samples, uint32_t n, void *d_rays_out, int num_cus, hipStream_t stream);
// rt_sensor_rays: the n = pixels x samples rt_ray records of pixels [first_pixel, ..) x samples [first_sample, first_sample + samples) of
// the sensor record `d_sensor` (device) -> `d_rays_out` (device, 32 B per record, 16-byte aligned)
hipError_t launch_sensor_rays(const WfSensor *d_sensor, uint32_t width, uint32_t height, uint32_t first_pixel, uint32_t first_sample, uint32_t samples, uint32_t n,
                              void *d_rays_out, int num_cus, hipStream_t stream);
// bytes of temporary storage rocPRIM's radix sort needs for `n` (key, slot) pairs
size_t wavefront_sort_temp_bytes(size_t n);
// rt_wf_extend.hip: closest hit over the binary tree
// closest-hit probe through the renderer's own kernels: `rays` (6 floats each, device) -> queue -> wf_extend (or wf_extend_packet)
// -> prim / bct (device). `L` carries the workspace (paths_in, hits, counters, stack_overflow, stats) and the traversal mode.
hipError_t launch_wavefront_cast(const DevScene &S, WfLaunch L, const float *rays, uint32_t n, bool packet, bool stats, uint32_t *prim, float *bct,
                                 hipStream_t stream);
// The camera-relative copy of a binary scene tree's records (WfLaunch::rel_nodes / rel_tris) for the camera position o[3]: one kernel on
// `stream`; `rel_nodes` has room for n_nodes records, `rel_tris` for bvh.n_tris.
hipError_t launch_camera_relative(const DevBvh &bvh, uint32_t n_nodes, const float *o, DevNode *rel_nodes, DevTri *rel_tris, int num_cus, hipStream_t stream);
// The compact records of a binary scene tree (DevBvh::compact) and the selector / valid bits in its DevNode::sel words, from the `n_nodes`
// final DevNode records: a memset and one kernel on `stream`; `compact` has room for n_nodes records.
hipError_t launch_derive_compact(DevNode *nodes, uint32_t n_nodes, DevNodeCompact *compact, int num_cus, hipStream_t stream);
// the closest-hit kernel of one bounce over the queue of `L`, on the grid the overflow workspace is sized for (L.stack_stride / 256 blocks):
// wf_extend, or wf_extend_packet for `packet` (coherent primary rays); the 8-wide tree's kernels for a scene that has one (below)
hipError_t launch_extend(const DevScene &S, const WfLaunch &L, bool packet, bool stats, hipStream_t stream);
// behind it, for a scene with analytic primitives: the nearer of (tree hit, primitive hit) for every queued ray (wf_extend_prims, grid-stride)
hipError_t launch_extend_prims(const DevScene &S, const WfLaunch &L, uint32_t blocks, hipStream_t stream);
// rt_wide.hip: the closest-hit kernel of scenes built with RT_BUILD_WIDE (same queue protocol as wf_extend)
// `packet`: the wave walks the tree once for its 64 consecutive rays (coherent primary rays), records through the scalar cache
hipError_t launch_extend_wide(const DevScene &S, const WfLaunch &L, bool packet, bool stats, int blocks, hipStream_t stream);
// rt_wf_shade.hip: wf_shade over the hits of `L`, in the instantiation the scene's lights and environment ask for
hipError_t launch_shade(const DevScene &S, const WfLaunch &L, bool stats, uint32_t blocks, hipStream_t stream);
// rt_accum.hip: the accumulators' per-round kernels (rt_abi.h rt_accum_*). `AccumRound` is the device state of one accumulator.
struct AccumRound {
    float *sum, *even_sum;     // [3 * pixels]
    uint32_t *count;           // [pixels]
    float *err;                // [pixels]: the last judge's err_p
    uint32_t *target;          // [pixels]: n_p the round brings pixel p to
    unsigned long long *scan_in, *scan; // [pixels]: (k > 0) << 32 | k per pixel, and its exclusive scan (entry index, sample offset)
    uint32_t *list_pix, *list_base, *list_off; // [pixels], [pixels], [pixels + 1]
    uint32_t *totals;          // [2] device: entries, samples of the planned list
    void *scan_temp;
    size_t scan_temp_bytes;
    uint32_t width, height;
};
size_t accum_scan_temp_bytes(uint32_t pixels);
// judge: err_p of every pixel, then target_p (round 0: max(n_p, min_samples); later: n_p + min(step, max - n_p) where active, n_p
// elsewhere). round0 != 0 computes no err and applies no window test.
hipError_t launch_accum_judge(const AccumRound &R, int round0, float threshold, uint32_t min_samples, uint32_t max_samples, uint32_t step,
                              hipStream_t stream);
// target_p = n_p + samples for every pixel (a progressive step)
hipError_t launch_accum_uniform(const AccumRound &R, uint32_t samples, hipStream_t stream);
// the list of entries (p, min(target_p - n_p, chunk)) with k > 0, in pixel order: exclusive scan + scatter; R.totals <- {entries, samples}
hipError_t launch_accum_plan(const AccumRound &R, uint32_t chunk, hipStream_t stream);
// fb[p] = S_p / (float)n_p (0 where n_p = 0)
hipError_t launch_accum_image(const AccumRound &R, float *fb, hipStream_t stream);
// the feature means (rt_accum_resolve_features): AS / n, NS / n, ZS / h; any output may be null
hipError_t launch_accum_feature_means(const AccumRound &R, const WfFeat &F, float *albedo, float *normal, float *depth, hipStream_t stream);
// the reads of an id table (rt_accum_resolve_labels, rt_accum_resolve_matte): device outputs, one word per pixel; `label` or `coverage` may be
// null. `set`: the matte's ids sorted ascending without duplicates, device, n_set >= 1.
hipError_t launch_accum_labels(const AccumRound &R, const WfIds &I, uint32_t *label, float *coverage, hipStream_t stream);
hipError_t launch_accum_matte(const AccumRound &R, const WfIds &I, const uint32_t *set, uint32_t n_set, float *matte, hipStream_t stream);
// the images of the group sums (rt_accum_resolve_light_group, rt_accum_resolve_light_mix): fb[p] = GS_g,p / (float)n_p, or per channel
// acc = +0; for g ascending: acc = acc + (GS_g,p / (float)n_p) * w[g][c]; a quotient is 0 where n_p = 0. The weights travel as a kernel argument.
struct LightMixWeights {
    float w[RT_LIGHT_GROUP_MAX][3];
};
hipError_t launch_accum_light_group(const AccumRound &R, const WfGroups &G, uint32_t group, float *fb, hipStream_t stream);
hipError_t launch_accum_light_mix(const AccumRound &R, const WfGroups &G, const LightMixWeights &w, float *fb, hipStream_t stream);
// the motion vectors (rt_accum_resolve_flow): flow[p] = FS_p / (float)m_p (RT_FLOW_MEAN) or NF_p (RT_FLOW_NEAREST), (0, 0) where m_p = 0;
// mask[p] = (float)m_p / (float)n_p, 0 where n_p = 0. Device outputs; either may be null.
hipError_t launch_accum_flow(const AccumRound &R, const WfFlow &F, uint32_t mode, float *flow, float *mask, hipStream_t stream);
// rt_lightmap.hip: rt_lightmap_points. The texel centres of a width x height atlas that the triangles (device arrays: 9 / 9 / 6 floats each) cover,
// as bake points in increasing texel order: owner per texel (integer atomicMin), exclusive scan, scatter. `owner` and `offs` have room for
// width * height words, `scan_temp` for lightmap_scan_temp_bytes(width * height); `count` (device, one word) receives the number of owned
// texels, of which the first `capacity` are written to `points_out` (32 B each) and `texels_out`.
size_t lightmap_scan_temp_bytes(size_t texels);
hipError_t launch_lightmap_points(const float *positions, const float *normals, const float *lm_uv, uint32_t n_tris, uint32_t width, uint32_t height, uint32_t *owner,
                                  uint32_t *offs, void *scan_temp, size_t scan_temp_bytes, void *points_out, uint32_t *texels_out, uint32_t capacity, uint32_t *count,
                                  int num_cus, hipStream_t stream);
// rt_denoise.hip: the a-trous filter of rt_accum_denoise (the rule: rt_abi.h). `D` is the filter's workspace, owned by the accumulator.
struct DenoiseBufs {
    RtF4 *sig[2]; // [pixels]: the working signal L, ping-pong
    RtF4 *den;    // [pixels]: den.rgb
    RtF4 *guide;  // [2 * pixels]: {N.xyz, Z}, {s, flags (u32 bits: 1 valid, 2 hit), 0, 0}
};
struct DenoiseOpt {
    uint32_t iterations, sharpness, demodulate;
    float sigma_color, sigma_depth;
};
hipError_t launch_denoise(const AccumRound &R, const WfFeat &F, const DenoiseBufs &D, const DenoiseOpt &O, float *fb, hipStream_t stream);
} // namespace rt
