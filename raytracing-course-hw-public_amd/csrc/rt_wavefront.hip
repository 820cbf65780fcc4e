// rt_wavefront.hip — the production render path (RT_RNG_DEVICE): a wavefront pipeline over PATHS.
//
// The reference renders pixel by pixel, sample by sample, bounce by bounce inside one recursive call chain
// (render_pixel -> trace_ray <-> shade, src/raytracer.h:555-627). On a 64-wide machine that nesting leaves most lanes
// idle: traversal lengths are heavy-tailed and a lane that finishes early waits for the wave's slowest ray before it may
// shade. Here a path = one (pixel, sample) and the recursion is cut into stages that each run over ALL live paths:
//
//   first stage : gen_ray (raytracer.h:527-538) for every path of the pass -> ray queue (wf_first_stage over the source of the pass's kind)
//   per bounce (ray_depth times):
//     wf_extend : closest hit (BVH::intersect_ray, bvh.h:195-235) for every queued ray. Persistent wavefronts; a lane
//                 whose traversal ends stores its hit and is refilled from the queue (wave ballot + prefix count out of
//                 the wave's private chunk of queue positions, one ticket atomic per 128-ray chunk), so the wave stays
//                 dense whatever the spread of traversal lengths. Bounces >= 1 walk the queue in a coherence-sorted order.
//     wf_shade  : one shade() level (raytracer.h:555-591) per hit: texture fetches, sampling, pdfs (incl. the light-BVH
//                 traversal), BRDF. Finished paths fold their (emission, scale) frames back-to-front (the Horner order of
//                 raytracer.h:588-590) and store the sample; surviving paths are COMPACTED into the next ray queue with
//                 a wave ballot + prefix sum (one atomic per wave).
//   last stage  : per pixel, the samples of the pass are added in sample order s = 0,1,2,... onto the running sum, so the
//                 float sum has exactly the reference's order (raytracer.h:621-626) although samples ran in parallel (wf_resolve, or
//                 what the pass's kind keeps its samples in).
// The two ends of a pass, which depend on its kind (rt_kernels.h WfPassKind), are rt_wf_stages.h. What runs between them for every kind alike
// is split by job: wf_extend and its kin with the closest-hit probe are rt_wf_extend.hip (the 8-wide tree: rt_wide.hip), wf_shade is
// rt_wf_shade.hip; this file has the small kernels between the stages (first-hit features, ids, motion vectors, group tags, the identity order, advance),
// the ray-order sort (the only user of rocPRIM) and the scheduler, launch_wavefront_pass, whose decisions are rt_wf_policy.h's.
//
// Every path owns an xoshiro128++ stream seeded from (seed, pixel, sample) and consumes it in the reference's draw
// order; the stream's state, the remaining depth and the count of pending frames travel with the ray through the queues
// (WfPath), so the image is independent of queue order, tiling and GPU count, and bit-identical to the persistent
// megakernel of rt_kernels.hip and to the CPU oracle in device-RNG mode.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/rt_flowspec.h"
#include "rt_kernels.h"
#include "rt_wf_policy.h"
#include "rt_wf_stages.h"

namespace {

// ------------------------------------------------------------------------------------------------ first-hit features
// A pass of a feature accumulator (rt_abi.h RT_ACCUM_FEATURES), after bounce 0's closest hits: the albedo, shading normal and distance of every
// primary ray's hit, from the shading record wf_shade is about to make of the same (ray, hit) pair (make_surf), one 32-byte record per path.
// At bounce 0 queue position i holds path i (wf_first_stage), and no order is in force. Counts nothing: the event counters are shade()'s.
__global__ __launch_bounds__(256) void wf_features(const DevScene S, const WfLaunch L, const WfFeat F) {
    __shared__ float s_lin[256];
    __shared__ float s_gam[256];
    s_lin[threadIdx.x] = S.lut_linear[threadIdx.x];
    s_gam[threadIdx.x] = S.lut_gamma[threadIdx.x];
    __syncthreads();
    LaneStats<false> st;
    const uint32_t n_in = L.counters[WF_CNT_IN];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += gridDim.x * blockDim.x) {
        const WfHead in = wf_load_head(L.paths_in + i);
        const Hit h = wf_load_hit(L.hits + i);
        RtF4 r0{0.f, 0.f, 0.f, 0.f}, r1{0.f, 0.f, 0.f, __uint_as_float(0u)};
        if (h.k != RT_NONE) {
            const Surf sf = make_surf<false>(S, h, in.o, in.d, s_lin, s_gam, st);
            r0 = RtF4{sf.color.r, sf.color.g, sf.color.b, h.t};
            r1 = RtF4{sf.shading_normal.x, sf.shading_normal.y, sf.shading_normal.z, __uint_as_float(1u)};
        }
        F.rec[2ull * in.id] = r0;
        F.rec[2ull * in.id + 1] = r1;
    }
}

// The ids of the same hits (rt_abi.h rt_accum_attach_ids), for a pass of an accumulator with ids: one u32 per path. Queue position i holds
// path i here, as for wf_features. PRIMITIVE is what wf_hits_out reports as `prim`; MATERIAL the material of that triangle or primitive;
// USER the accumulator's table at `prim`.
__global__ __launch_bounds__(256) void wf_ids(const DevScene S, const WfLaunch L, const WfIds I) {
    const uint32_t n_in = L.counters[WF_CNT_IN];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += gridDim.x * blockDim.x) {
        const WfHead in = wf_load_head(L.paths_in + i);
        const uint32_t k = wf_load_hit(L.hits + i).k;
        uint32_t id = RT_ID_MISS;
        if (k != RT_NONE) {
            const bool analytic = (k & RT_PRIM_FLAG) != 0u;
            const uint32_t pi = k & ~RT_PRIM_FLAG;
            if (I.kind == RT_ID_MATERIAL) {
                id = analytic ? S.prims[pi].material_id : S.attrs[k].material;
            } else {
                id = analytic ? S.n_triangles + pi : S.scene.tris[k].prim;
                if (I.kind == RT_ID_USER)
                    id = I.table[id];
            }
        }
        I.rec[in.id] = id;
    }
}

// The motion vectors of the same hits (rt_abi.h rt_accum_attach_flow), for a pass of an accumulator with flow: one 16-byte record per path.
// Queue position i holds path i here, as for wf_features. The arithmetic is include/rt_flowspec.h's, which the CPU tests read too. Both views
// are wave-uniform: scalar loads, and the kind a scalar branch, as in sensor_ray. The two gathers of 36 bytes per triangle hit, one per key
// at DevTri::prim, are the kernel's whole cost; an analytic primitive and an accumulator whose triangles do not move gather nothing.
DEV rt_flow_view wf_flow_view(const WfSensor &sn) {
    rt_flow_view v;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        v.P[c] = sn.pos[c], v.R[c] = sn.right[c], v.U[c] = sn.up[c], v.F[c] = sn.fwd[c];
    v.tan_x = sn.tan_x, v.tan_y = sn.tan_y;
    v.half_fov = sn.half_fov;
    v.half_width = sn.half_width, v.half_h = sn.half_h;
    v.kind = sn.kind;
    return v;
}
__global__ __launch_bounds__(256) void wf_flow(const DevScene S, const WfLaunch L, const WfFlow Fl) {
    const rt_flow_view v0 = wf_flow_view(L.sensors[0]), v1 = wf_flow_view(*Fl.sensor1); // an accumulator has one camera
    const uint32_t n_in = L.counters[WF_CNT_IN];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_in; i += gridDim.x * blockDim.x) {
        const WfHead in = wf_load_head(L.paths_in + i);
        const Hit h = wf_load_hit(L.hits + i);
        RtF4 r{0.f, 0.f, 0.f, __uint_as_float(0u)};
        if (h.k != RT_NONE) {
            float X0[3], X1[3];
            if ((h.k & RT_PRIM_FLAG) != 0u || Fl.n_triangles == 0u) {
                const float o[3] = {in.o.x, in.o.y, in.o.z}, d[3] = {in.d.x, in.d.y, in.d.z};
                rt_flow_ray_point(o, d, h.t, X0);
                X1[0] = X0[0], X1[1] = X0[1], X1[2] = X0[2];
            } else {
                const size_t at = 9ull * S.scene.tris[h.k].prim;
                float k0[9], k1[9];
#pragma unroll
                for (int j = 0; j < 9; ++j)
                    k0[j] = Fl.key[0][at + j], k1[j] = Fl.key[1][at + j];
                rt_flow_tri_point(k0, h.b, h.c, X0);
                rt_flow_tri_point(k1, h.b, h.c, X1);
            }
            float dx, dy;
            if (rt_flow_sample(&v0, &v1, L.width, L.height, X0, X1, &dx, &dy))
                r = RtF4{dx, dy, h.t, __uint_as_float(1u)};
        }
        Fl.rec[in.id] = r;
    }
}

// ------------------------------------------------------------------------------------------------ light-group tags
// A pass of an accumulator with light groups (rt_abi.h rt_accum_attach_light_groups; WfGroups), at EVERY bounce, between the closest hits and
// wf_shade: whose emission the frame (or the terminal value) that wf_shade is about to make of this (ray, hit) pair is. It reads what wf_shade
// reads, the hit at queue position jq and the head of the ray that position stands for, and writes one byte at the head's own frame level:
// the group of the hit's material, the background's group for a miss, WF_GROUP_NONE for neither. Counts nothing.
__global__ __launch_bounds__(256) void wf_group_tags(const DevScene S, const WfLaunch L, const WfGroups Gr) {
    const uint32_t n_in = L.counters[WF_CNT_IN];
    for (uint32_t jq = blockIdx.x * blockDim.x + threadIdx.x; jq < n_in; jq += gridDim.x * blockDim.x) {
        const uint32_t k = wf_load_hit(L.hits + jq).k;
        const WfHead in = wf_load_head(L.paths_in + wf_order_slot(L, jq));
        uint32_t tag = Gr.background;
        if (k != RT_NONE)
            tag = Gr.material_group[(k & RT_PRIM_FLAG) != 0u ? S.prims[k & ~RT_PRIM_FLAG].material_id : S.attrs[k].material];
        Gr.tag[wf_fold_index(L.n_paths, in.nb, in.id)] = (uint8_t)tag;
    }
}

// The order of a bounce no sort runs over (sorting off, or a queue below the sort's threshold): the identity over the dense ray index, as the
// physical slot of paths_in (wf_shade's sub-queue regions, WF_STRIPES), straight to sort_vals[1]. No record is read: WfLaunch::order_classed = 0.
// A bounce that IS sorted needs no such pass: its producer wrote key and slot at every filled physical slot (wf_shade, WfLaunch::emit_keys; the
// key is rt_ray_key.h's), the unfilled ends of the regions hold pad keys, and the sort runs over the physical positions.
__global__ __launch_bounds__(256) void wf_sort_keys(const WfLaunch L) {
    __shared__ uint32_t s_run[WF_STRIPES + 1u];
    const uint32_t n = L.counters[WF_CNT_IN], n_slots = L.counters[WF_CNT_SLOTS];
    if (threadIdx.x <= WF_STRIPES)
        s_run[threadIdx.x] = L.stripes[WF_STRIPES * WF_STRIPE_WORDS + threadIdx.x];
    __syncthreads();
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        uint32_t pos = j;
        if (n_slots != 0u) { // run k holds dense indices [s_run[k], s_run[k+1])
            uint32_t k = 0;
#pragma unroll
            for (uint32_t step = WF_STRIPES / 2u; step != 0u; step >>= 1)
                if (s_run[k + step] <= j)
                    k += step;
            pos = wf_stripe_base(k, n_slots) + (j - s_run[k]);
        }
        L.sort_vals[1][j] = pos;
    }
}

// next bounce: the out queue becomes the in queue (the host swaps the pointers). The sub-queue fill counters turn into the
// dense prefix run_start[] the ray-order pass reads, and are cleared for the next wf_shade. One wave.
__global__ __launch_bounds__(64) void wf_advance(uint32_t *counters, uint32_t *stripes) {
    const uint32_t k = threadIdx.x; // == WF_STRIPES lanes
    const uint32_t c = stripes[k * WF_STRIPE_WORDS];
    uint32_t incl = c;
#pragma unroll
    for (uint32_t d = 1; d < WF_STRIPES; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (k >= d)
            incl += up;
    }
    uint32_t *run_start = stripes + WF_STRIPES * WF_STRIPE_WORDS;
    run_start[k] = incl - c;
    stripes[k * WF_STRIPE_WORDS] = 0u;
    if (k == WF_STRIPES - 1u) {
        run_start[WF_STRIPES] = incl;
        counters[WF_CNT_SLOTS] = (counters[WF_CNT_IN] + 63u) >> 6; // wave slots of the launch that just wrote the new in-queue
        counters[WF_CNT_IN] = incl;
        counters[WF_CNT_TICKET] = 0;
    }
    if (k < 8u)
        counters[WF_CNT_XCD + k * WF_CNT_XCD_STRIDE] = 0u;
}

} // namespace

namespace rt {

// the first stage of the pass's source (rt_wf_stages.h)
static hipError_t launch_first_stage(const DevScene &S, const WfLaunch &L, const WfPassKind &kind, bool stats, dim3 grid, hipStream_t stream) {
    return with_bools([&](auto ST, auto ED) {
        switch (kind.source()) {
        case WfPassKind::LIST:
            return RT_LAUNCH_CHECKED((wf_first_stage<ST, ED, WfFromList>), grid, dim3(256), 0, stream, S, L, kind.entries());
        case WfPassKind::RAYS:
            return RT_LAUNCH_CHECKED((wf_first_stage<ST, ED, WfFromRays>), grid, dim3(256), 0, stream, S, L, kind.ray_buffer());
        case WfPassKind::BAKE:
            return RT_LAUNCH_CHECKED((wf_first_stage<ST, ED, WfFromBake>), grid, dim3(256), 0, stream, S, L, kind.bake_points());
        default:
            return RT_LAUNCH_CHECKED((wf_first_stage<ST, ED, WfFromCameras>), grid, dim3(256), 0, stream, S, L, WfFromCameras::Arg{});
        }
    }, stats, S.env.texels != nullptr && S.env.marg != nullptr);
}

// the last stage of the pass's kind: where the folded samples of the pass go
static hipError_t launch_last_stage(const WfLaunch &L, const WfPassKind &kind, const WfPassStep &step, int num_cus, hipStream_t stream) {
    const dim3 block(256);
    const int first = step.first_pass ? 1 : 0, last = step.last_pass ? 1 : 0;
    if (kind.source() == WfPassKind::LIST) { // the feature sums, the id tables, the group sums and the flow go before the sums: they read the entry's base count from the list
        const WfAccum &A = kind.entries();
        const WfLayers keep = kind.layers();
        const dim3 grid(wf_grid_items(A.n_entries));
        if (keep.features)
            WF_LAUNCH(wf_resolve_features, grid, block, 0, stream, A, *keep.features);
        if (keep.ids)
            WF_LAUNCH(wf_resolve_ids, grid, block, 0, stream, A, *keep.ids);
        if (keep.groups)
            WF_LAUNCH(wf_resolve_groups, grid, block, 0, stream, A, *keep.groups, L.n_paths);
        if (keep.flow)
            WF_LAUNCH(wf_resolve_flow, grid, block, 0, stream, A, *keep.flow);
        WF_LAUNCH(wf_resolve_list, grid, block, 0, stream, L, A);
    } else if (kind.source() == WfPassKind::BAKE) { // the fold the bake's kind asks for, one lane per (point, k)
        const WfBake &B = kind.bake_points();
        const uint64_t lanes = (uint64_t)L.pass_pixels * (B.kind == RT_BAKE_SH9 ? 9u : 1u);
        WF_LAUNCH(wf_resolve_bake, dim3(wf_grid_stride(lanes, num_cus, 64u)), block, 0, stream, L, B, first, last);
    } else { // cameras, a caller's rays: the image, or the outputs as a one-row image
        WF_LAUNCH(wf_resolve, dim3(wf_grid_items(L.pass_pixels)), block, 0, stream, L, first, last);
    }
    return hipSuccess;
}

// Bounce b >= 1 walks its queue through an order, L.order: the ray-order sort over the PHYSICAL positions of the queue (its producer had at
// most `bound` rays = sort_span(bound) / 64 wave slots, wrote key and slot at every position it filled and found pads at the others:
// WfPassPolicy::emits_keys), or, unsorted, the identity from dense ray index to slot of paths_in (wf_shade's sub-queue regions)
static hipError_t launch_ray_order(WfLaunch &L, bool sorted, uint32_t bound, int num_cus, hipStream_t stream) {
    if (sorted) {
        size_t tmp = L.sort_temp_bytes;
        hipError_t se = rocprim::radix_sort_pairs(L.sort_temp, tmp, L.sort_keys[0], L.sort_keys[1], L.sort_vals[0], L.sort_vals[1], WfPassPolicy::sort_span(bound), 0u, RT_RAY_KEY_BITS, stream);
        if (se != hipSuccess)
            return se;
    } else {
        WF_LAUNCH(wf_sort_keys, dim3(wf_grid_stride(bound, num_cus, 16u)), dim3(256), 0, stream, L);
    }
    L.order = L.sort_vals[1];
    L.order_classed = sorted ? 1u : 0u;
    return hipSuccess;
}

// Device words on their way to the host without ever idling the device: a copy to pinned words with an event behind it; whoever needs the
// words later waits for that event alone, with everything queued since still ahead of the device.
struct HostWords {
    const WfHostSync *hs;
    hipStream_t stream;
    hipError_t send(uint32_t event, uint32_t word, const void *src, size_t bytes) const {
        if (hipError_t e = hipMemcpyAsync(hs->counts + word, src, bytes, hipMemcpyDeviceToHost, stream); e != hipSuccess)
            return e;
        return hipEventRecord(hs->events[event], stream);
    }
    hipError_t wait(uint32_t event) const { return hipEventSynchronize(hs->events[event]); }
};

// One pass of the pipeline, stream-ordered: first stage, ray_depth x (order, extend, shade, advance), fold, last stage. The host waits only
// for the words it reads back (below). `L.paths_in/paths_out` are swapped locally per bounce.
hipError_t launch_wavefront_pass(const DevScene &S, WfLaunch L, const WfPassKind &kind, const WfPassStep &step, bool stats, int num_cus, hipStream_t stream,
                                 EventPool *extend_events, unsigned long long *packet_census_out, const WfHostSync *host_sync) {
    const dim3 block(256), path_grid(wf_grid_stride(L.n_paths, num_cus, 16u));
    const uint32_t shade_blocks = (uint32_t)num_cus * RT_SHADE_BLOCKS_PER_CU;
    const WfLayers keep = kind.layers();
    if (!step.time_extends)
        extend_events = nullptr;
    hipError_t e = hipMemsetAsync(L.counters, 0, sizeof(uint32_t) * WF_CNT_WORDS, stream);
    if (e != hipSuccess)
        return e;
    if ((e = hipMemsetAsync(L.stripes, 0, sizeof(uint32_t) * WF_STRIPE_BUF_WORDS, stream)) != hipSuccess)
        return e;
    const bool packet = L.use_packet != 0u && L.packet_census != nullptr;
    if (packet && (e = hipMemsetAsync(L.packet_census, 0, 2 * sizeof(unsigned long long), stream)) != hipSuccess)
        return e;
    if (packet_census_out)
        packet_census_out[0] = packet_census_out[1] = 0ull;
    if ((e = launch_first_stage(S, L, kind, stats, path_grid, stream)) != hipSuccess)
        return e;
    // Queue sizes reach the host one bounce LATE and without ever idling the device: after bounce b's wf_advance the size of
    // queue b + 1 is copied to pinned word b + 1 and an event is recorded; bounce b + 2 waits for THAT event — by then bounce
    // b + 1's kernels are queued behind it, so the device has a whole bounce of work while the host looks. The host needs the
    // size only as an upper bound (grid of the ray-order pass, length of the sort, "nothing left": stop): the kernels read the
    // exact size from device memory. (Round 2 synchronised the stream once per bounce: eight idle gaps per pass.)
    const WfHostSync *hs = L.sort_mode != 0u || (packet && packet_census_out) ? host_sync : nullptr;
    if (hs && (!hs->counts || !hs->events || hs->n_events < (int)L.ray_depth + 1))
        hs = nullptr;
    const HostWords host{hs, stream};
    // the per-bounce size read-back (one host wait per bounce from bounce 2 on) is only worth its latency where a sort follows; an unsorted
    // pass (a small one, rt_scene.cpp; or RT_SORT_OFF) is queued in one go and only the packet census, if any, is waited for once
    const WfPassPolicy policy{L.n_paths, L.ray_depth, hs && L.sort_mode != 0u};
    // the packet kernel's census of bounce 0 -> pinned words behind event 0; read at bounce 2, when its copy is two bounces behind the queue
    // head, or behind the loop (ray_depth <= 2: the rest of the pass is queued behind it by then)
    bool census_pending = false;
    auto read_census = [&]() -> hipError_t {
        if (hipError_t ce = host.wait(0); ce != hipSuccess)
            return ce;
        std::memcpy(packet_census_out, hs->counts + WF_HOST_CENSUS_WORD, 2 * sizeof(unsigned long long));
        census_pending = false;
        return hipSuccess;
    };
    for (uint32_t b = 0; b < L.ray_depth; ++b) {
        if (census_pending && b == 2 && (e = read_census()) != hipSuccess)
            return e;
        if (policy.waits_for_size(b) && (e = host.wait(b - 1)) != hipSuccess) // size of queue b - 1, an upper bound of queue b
            return e;
        const uint32_t bound = policy.bound(b, hs ? hs->counts : nullptr); // of the queue entering this bounce
        if (policy.ends_pass(b, bound))
            break;
        L.order = nullptr, L.order_classed = 0u; // primary rays: dense and coherent as generated
        if (b > 0 && (e = launch_ray_order(L, policy.sorted(b, bound), bound, num_cus, stream)) != hipSuccess)
            return e;
        // time the dominant kernel per launch (bench.py roofline): HIP events on the launch stream, taken from the scene's
        // pool (created once, reused by every render)
        hipEvent_t e0 = extend_events ? extend_events->next() : nullptr;
        hipEvent_t e1 = e0 ? extend_events->next() : nullptr;
        if (e0 && e1)
            (void)hipEventRecord(e0, stream);
        if ((e = launch_extend(S, L, b == 0 && packet, stats, stream)) != hipSuccess)
            return e;
        if (e0 && e1)
            (void)hipEventRecord(e1, stream);
        if (S.n_prims && (e = launch_extend_prims(S, L, shade_blocks, stream)) != hipSuccess)
            return e;
        if (b == 0 && keep.features) // a feature accumulator's pass: the primary rays' first hits are final here
            WF_LAUNCH(wf_features, dim3(shade_blocks), block, 0, stream, S, L, *keep.features);
        if (b == 0 && keep.ids) // ... and so are their ids
            WF_LAUNCH(wf_ids, dim3(shade_blocks), block, 0, stream, S, L, *keep.ids);
        if (b == 0 && keep.flow) // ... and their motion vectors
            WF_LAUNCH(wf_flow, dim3(shade_blocks), block, 0, stream, S, L, *keep.flow);
        if (keep.groups) // light groups: at every bounce, whose emission the frame or terminal value wf_shade makes of this hit is
            WF_LAUNCH(wf_group_tags, dim3(shade_blocks), block, 0, stream, S, L, *keep.groups);
        // May the next bounce be sorted (WfPassPolicy::emits_keys)? Then this wf_shade writes the sort's input itself, key and slot at the
        // physical slot of every ray it makes, and every slot it leaves empty (the ends of the 64 sub-queue regions) must already hold a pad:
        // RT_RAY_KEY_PAD in the compared bits, behind every real key wherever it stands. (A byte fill of the range at HBM rate, a few tens of
        // microseconds; the bounce's own sort has read sort_keys[0] by now: it is earlier in the stream.)
        L.emit_keys = policy.emits_keys(b, bound) ? 1u : 0u;
        if (L.emit_keys && (e = hipMemsetAsync(L.sort_keys[0], 0xFF, sizeof(uint32_t) * WfPassPolicy::pad_span(bound), stream)) != hipSuccess)
            return e;
        if ((e = launch_shade(S, L, stats, shade_blocks, stream)) != hipSuccess)
            return e;
        WF_LAUNCH(wf_advance, dim3(1), dim3(64), 0, stream, L.counters, L.stripes);
        if (hs && b == 0 && packet && packet_census_out) {
            if ((e = host.send(0, WF_HOST_CENSUS_WORD, L.packet_census, 2 * sizeof(unsigned long long))) != hipSuccess)
                return e;
            census_pending = true;
        }
        if (policy.records_size(b) && (e = host.send(b + 1, b + 1, L.counters + WF_CNT_IN, sizeof(uint32_t))) != hipSuccess) // size of queue b + 1, for bounce b + 2
            return e;
        WfPath *t = L.paths_in;
        L.paths_in = L.paths_out;
        L.paths_out = t;
    }
    if (keep.groups) // before wf_fold, which overwrites the terminal values in sample_out
        WF_LAUNCH(wf_fold_groups, path_grid, block, 0, stream, L, *keep.groups);
    WF_LAUNCH(wf_fold, path_grid, block, 0, stream, L);
    if (census_pending && (e = read_census()) != hipSuccess)
        return e;
    return launch_last_stage(L, kind, step, num_cus, stream);
}

hipError_t launch_sensor_rays(const WfSensor *d_sensor, uint32_t width, uint32_t height, uint32_t first_pixel, uint32_t first_sample, uint32_t samples, uint32_t n,
                              void *d_rays_out, int num_cus, hipStream_t stream) {
    return RT_LAUNCH_CHECKED(wf_sensor_rays, dim3(wf_grid_stride(n, num_cus, 16u)), dim3(256), 0, stream, d_sensor, width, height, first_pixel, first_sample, samples, n,
                             static_cast<uint4 *>(d_rays_out));
}

hipError_t launch_bake_rays(const WfBake &B, uint32_t samples, uint32_t n, void *d_rays_out, int num_cus, hipStream_t stream) {
    return RT_LAUNCH_CHECKED(wf_bake_rays, dim3(wf_grid_stride(n, num_cus, 16u)), dim3(256), 0, stream, B, samples, n, static_cast<uint4 *>(d_rays_out));
}

size_t wavefront_sort_temp_bytes(size_t n) {
    size_t tmp = 0;
    uint32_t *k = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, tmp, k, k, k, k, n, 0u, RT_RAY_KEY_BITS, (hipStream_t) nullptr);
    return tmp;
}

} // namespace rt
