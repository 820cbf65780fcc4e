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
// The two ends of a pass, which depend on its kind (rt_kernels.h WfPassKind), are rt_wf_stages.h; this file has what runs between them for
// every kind alike (extend, shade, sort, advance), the closest-hit probe and the launchers.
//
// Every path owns an xoshiro128++ stream seeded from (seed, pixel, sample) and consumes it in the reference's draw
// order; the stream's state, the remaining depth and the count of pending frames travel with the ray through the queues
// (WfPath), so the image is independent of queue order, tiling and GPU count, and bit-identical to the persistent
// megakernel of rt_kernels.hip and to the CPU oracle in device-RNG mode.
#include <algorithm>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "rt_dev_queue.h"
#include "rt_dev_shade.h"
#include "rt_dev_stack.h"
#include "rt_kernels.h"
#include "rt_ray_key.h"
#include "rt_wf_records.h"
#include "rt_wf_stages.h"

namespace {

#ifndef RT_EXT_WAVES_PER_SIMD
#define RT_EXT_WAVES_PER_SIMD 6 /* <= 80 VGPRs; measured best with RT_EXT_LDS_DEPTH 6 (tools_sweep.sh) */
#endif
#ifndef RT_EXT_LDS_DEPTH
#define RT_EXT_LDS_DEPTH 6 /* LDS part of the traversal stack in wf_extend: 6 -> 26 KB/block -> 6 blocks (24 waves) per CU */
#endif
#ifndef RT_EXT_GB_LDS_DEPTH
#define RT_EXT_GB_LDS_DEPTH 9 /* global-best traversal: 8-byte frames {ref, d_far} -> 9 positions in the LDS the reference traversal's 6 x 12 B take */
#endif
#ifndef RT_SHADE_WAVES_PER_SIMD
#define RT_SHADE_WAVES_PER_SIMD 4
#endif
#ifndef RT_SHADE_BLOCKS_PER_CU
#define RT_SHADE_BLOCKS_PER_CU 8 /* grid of the grid-stride kernels (wf_shade, wf_extend_prims) */
#endif
#ifndef RT_SHADE_LDS_DEPTH
#define RT_SHADE_LDS_DEPTH 4 /* only the light-BVH traversal of bvh_mix_dist::pdf uses a stack in wf_shade */
#endif
using ShadeStack = StackMemT<RT_SHADE_LDS_DEPTH>;
#ifndef RT_EXT_CHUNK
#define RT_EXT_CHUNK 64u /* queue positions a wave takes per ticket atomic (128 until the tickets were partitioned: with eight heads the atomics are cheap
                            and the last ticket of a part is one batch of work, not two: + 0.7 % S-sponza, + 1 % S-10M, profiles/r03_variants.txt item 21) */
#endif
#ifndef RT_EXT_REFILL_MIN
#define RT_EXT_REFILL_MIN 16 /* refill a wave's idle lanes once this many have finished (a refill stalls the wave on the ray loads) */
#endif

// ------------------------------------------------------------------------------------------------ extend
// Closest hit for every queued ray. Two kinds of work alternate inside a wave instead of being interleaved:
//   * node steps   : lanes standing on an inner node test its two child boxes (trav_step_inner_fast; trav_step_core for a
//                    wave with a guarded ray or a big-leaf walker), lanes that reached a leaf wait;
//   * leaf batches : once enough lanes wait on leaves (or nobody is left on inner nodes) the wave tests ALL their
//                    triangles together: the (ray, triangle) pairs of the waiting lanes are laid out densely over the
//                    64 lanes (prefix sum of the leaf sizes), each lane fetches "its" ray from the owning lane with
//                    cross-lane reads and runs one triangle test; a leaf's result is the minimum of a 64-bit key
//                    (t bits, triangle index) reduced with LDS atomics, i.e. smallest t and, on equal t, the
//                    lowest triangle index — exactly the leaf loop's strict-less replacement order (bvh.h:200-204,132).
// This removes the inner-node / triangle divergence of a one-record-per-lane step (about 58 % / 42 % of the lanes) and
// packs the triangle tests: a wave does ~40 node tests or ~48 triangle tests per pass instead of ~27 + ~20.
// (The batch itself is coop_tri_batch, rt_dev_trav.h; here: a lane contributes its whole leaf, records are DevTri in leaf order.)
template <bool STATS> DEV void leaf_batch(Trav &T, const DevBvh &bvh, bool at_leaf, const CoopLds<float2> &lds, LaneStats<STATS> &st) {
    coop_tri_batch<RT_LEAF_COOP_MAX>(
        at_leaf, at_leaf ? RT_LEAF_CNT(T.cur) : 0u, T.cur & RT_LEAF_BEGIN_MASK, T.o, T.d, bvh.tris, lds, [](int t) { return (uint32_t)t; },
        [](uint32_t k0, uint32_t e) { return k0 + e; }, st);
    if (at_leaf) {
        st.node(); // one BVH::intersect_ray invocation on the leaf node
        float t;
        uint32_t k;
        float2 bc;
        if (coop_result(lds, t, k, bc)) {
            hit_take(T.best, k, bc.x, bc.y, t);
            T.t_loc = fminf(T.t_loc, t);
        }
        T.cur = T_POP; // unwound by the caller's trav_pop_wave
    }
}

#ifndef RT_EXT_LEAF_MIN
#define RT_EXT_LEAF_MIN 20 /* run a leaf batch once this many lanes wait on a leaf */
#endif
#ifndef RT_EXT_SPARSE_MAX
#define RT_EXT_SPARSE_MAX 32 /* a wave whose queue is used up drains eagerly once this many lanes or fewer still walk (swept 0 / 4 .. 64:
                                profiles/camera_relative_sparse_drain.txt) */
#endif

// One record for every `stepper` lane of the wave. The common wave: every stepping lane is on an inner node with the fast-division
// guarantees -> straight-line node step; a wave with a big-leaf walker or a guarded ray takes the general step.
template <bool STATS, bool GB, class STK> DEV void node_step(Trav &T, const DevBvh &bvh, STK &stk, bool stepper, LaneStats<STATS> &st) {
    const bool plain = (T.cur & RT_LEAF_FLAG) == 0 && T.fast;
    if (__ballot(stepper && !plain) == 0ull) {
        if (stepper) {
            trav_step_inner_fast<STATS, GB>(T, bvh, stk, EPS, st);
        }
    } else if (stepper) {
        trav_step_core<STATS, GB>(T, bvh, stk, EPS, st);
    }
}

template <bool STATS, bool GB> __global__ __launch_bounds__(256, RT_EXT_WAVES_PER_SIMD) void wf_extend(const DevScene S, const WfLaunch L) {
    constexpr int DEPTH = GB ? RT_EXT_GB_LDS_DEPTH : RT_EXT_LDS_DEPTH, WORDS = GB ? 2 : 3;
    __shared__ uint32_t s_stack[STACK_LDS_DWORDS(DEPTH, WORDS)];
    __shared__ uint16_t s_owner_all[4][64 * RT_LEAF_COOP_MAX + RT_LEAF_COOP_MAX]; // + overshoot of the unpredicated owner stores
    __shared__ unsigned long long s_min_all[4][64];
    __shared__ float2 s_bc_all[4][64];
    const uint32_t wave = threadIdx.x >> 6;
    const CoopLds<float2> s_coop{s_owner_all[wave], s_min_all[wave], s_bc_all[wave]};
    LaneStats<STATS> st;
    RT_DECLARE_RING_STACK_W(stk, DEPTH, WORDS, s_stack, L.stack_overflow, L.stack_stride);
    const uint32_t n_in = L.counters[WF_CNT_IN];
    Trav T;
    T.cur = T_DONE;
    T.sp = 0;
    uint32_t slot = RT_NONE;
    bool exhausted = n_in == 0; // wave-uniform
    uint32_t q_lo = 0, q_hi = 0; // this wave's private range of queue positions
    TicketState tks = ticket_init();
    for (;;) {
        const int n_idle = ticket_refill(L.counters, n_in, (uint32_t)RT_EXT_CHUNK, RT_EXT_REFILL_MIN, T.cur == T_DONE, exhausted, q_lo, q_hi, tks, [&](uint32_t jq) {
            const WfRay ray = wf_load_ray(L.paths_in + wf_order_slot(L, jq)); // coherence-sorted processing order
            slot = jq; // the hit goes to the queue POSITION (see WfLaunch::hits)
            trav_init_stored<GB>(T, S.scene, ray.o, ray.d, ray.r, ray.fast);
            stk.reset();
            if (T.cur == T_DONE) // no geometry at all: immediate miss
                wf_store_hit(L.hits + jq, wf_miss());
        });
        // Bounded unwind: ONE stack pop per trip for every lane that has to unwind (a lane whose pop ends in a pruned far
        // child pops again next trip and sits out one node step: ~1 in 5 unwinding lanes). The unwind used to be a loop that
        // ran until no lane of the wave was left in T_POP: 1.2 iterations per trip at ~7 of 64 lanes, each a full LDS round
        // trip, plus the loop's own header and exit code — 22 % of the kernel's wave cycles (profiles/r02_extend_sections.txt).
        // (Tried and not kept: issuing the pop's LDS reads here and consuming them only behind the node fetch — 3 more live
        // VGPRs and the extra predicate traffic cost more than the hidden LDS round trip: 233.7 vs 238.5 Msamples/s.)
        const bool was_live = T.cur != T_DONE;
        trav_pop_once<GB>(T, stk);
        if (was_live && T.cur == T_DONE)
            wf_store_hit(L.hits + slot, T.best);
        const bool active = T.cur != T_DONE;
        const bool popping = T.cur == T_POP; // note: T_POP has the leaf bit set, it must be told apart first
        const bool at_leaf = active && !popping && (T.cur & RT_LEAF_FLAG) != 0 && RT_LEAF_CNT(T.cur) != 0;
        const bool stepper = active && !popping && !at_leaf; // inner node, or a big leaf walked triangle by triangle
        const unsigned long long lm = __ballot(at_leaf), sm = __ballot(stepper);
        if ((lm | sm) == 0ull) {
            if (__ballot(popping) != 0ull)
                continue; // only unwinding lanes left: pop again
            if (exhausted)
                break;
            continue;
        }
        if (sm == 0ull || __popcll(lm) >= RT_EXT_LEAF_MIN) {
            leaf_batch<STATS>(T, S.scene, at_leaf, s_coop, st);
            // The one place that looks whether the wave has become sparse: a scalar test on the trips that ran a batch (a sparse wave runs
            // one every few trips: its steppers are few), so the loop head and the node step stay what they were. n_idle is this trip's count
            // from before the unwind: with the queue used up lanes only ever finish, so it can only be too small. (A block is 4 full waves.)
            if (exhausted && n_idle >= 64 - RT_EXT_SPARSE_MAX)
                break; // -> the sparse drain behind the loop
        } else {
            node_step<STATS, GB>(T, S.scene, stk, stepper, st);
        }
    }
    // Sparse drain: the queue is used up and at most RT_EXT_SPARSE_MAX lanes still walk. Nothing is left to keep busy, so the throughput
    // policies of the loop above (wait for 20 leaves, one pop per trip, a leaf batch OR a node step) only lengthen the chain of the wave's
    // slowest ray, and that chain is the launch's tail. A trip here unwinds until no lane is left in T_POP, tests the leaves of the lanes
    // that stand on one at once, unwinds again, and steps every lane that stands on an inner node. Each lane runs the same state machine in
    // the same order as above: hits and counters are unchanged by construction.
    bool live = T.cur != T_DONE;
    auto unwind = [&]() {
        trav_pop_wave<GB>(T, stk);
        if (live && T.cur == T_DONE) {
            wf_store_hit(L.hits + slot, T.best);
            live = false;
        }
    };
    for (;;) {
        unwind();
        if (__ballot(live) == 0ull)
            break;
        const bool at_leaf = live && (T.cur & RT_LEAF_FLAG) != 0 && RT_LEAF_CNT(T.cur) != 0; // (no lane is in T_POP here)
        if (__ballot(at_leaf) != 0ull) {
            leaf_batch<STATS>(T, S.scene, at_leaf, s_coop, st);
            unwind();
        }
        // an inner node, or a big leaf walked triangle by triangle; a lane the unwind has just put on a small leaf waits one trip
        const bool stepper = live && !((T.cur & RT_LEAF_FLAG) != 0 && RT_LEAF_CNT(T.cur) != 0);
        if (__ballot(stepper) != 0ull)
            node_step<STATS, GB>(T, S.scene, stk, stepper, st);
    }
    st.flush(L.stats);
}

// ------------------------------------------------------------------------------------------------ extend: coherent packets
// Primary rays. A wave's 64 queue positions are 64 samples of one pixel (or a few neighbouring pixels): rays that visit almost
// the same nodes. wf_extend lets its lanes drift apart (each lane refills on its own), so it pays one vector-L1 access per lane
// and 16-byte piece for them like for any other ray, and the L1 access rate is its roof (profiles/r02_l1_roof.txt). Here the
// wave stays a packet: all 64 rays start together, and every trip serves ONE record — the smallest pending node or leaf
// reference over the lanes (inner nodes before leaves, earlier nodes first, so stragglers catch up and lanes re-join) —
// fetched once through the scalar cache and applied by the lanes standing on it. Each lane still runs its own traversal
// state machine (trav_inner_apply / the leaf loop of trav_step_core / trav_pop_once, its own stack, its own near/far order
// and pruning), only WHEN a lane advances is decided per wave: results, order of strict-less replacements and counters are
// the per-lane kernel's by construction. No vector loads on the traversal path at all.
#ifndef RT_PKT_CHUNK
#define RT_PKT_CHUNK 256u /* queue positions per ticket atomic (4 packets) */
#endif
// REL: the pass's primary rays all start at ONE camera position, bit for bit, and WfLaunch::rel_nodes / rel_tris hold the tree's records with
// that position folded in (wf_camera_relative below): the trips fetch those and skip what a lane would compute from the origin. The host
// decides (rt_render.cpp launch_pass); the kernel never compares origins.
template <bool STATS, bool GB, bool REL> __global__ __launch_bounds__(256, RT_EXT_WAVES_PER_SIMD) void wf_extend_packet(const DevScene S, const WfLaunch L) {
    constexpr int DEPTH = GB ? RT_EXT_GB_LDS_DEPTH : RT_EXT_LDS_DEPTH, WORDS = GB ? 2 : 3;
    __shared__ uint32_t s_stack[STACK_LDS_DWORDS(DEPTH, WORDS)];
    LaneStats<STATS> st;
    RT_DECLARE_RING_STACK_W(stk, DEPTH, WORDS, s_stack, L.stack_overflow, L.stack_stride);
    const uint32_t n_in = L.counters[WF_CNT_IN];
    const uint32_t lane = threadIdx.x & 63u;
    const DevNode *const nodes = REL ? L.rel_nodes : S.scene.nodes;
    const DevTri *const tris = REL ? L.rel_tris : S.scene.tris;
    Trav T = trav_idle<GB>();
    unsigned long long n_trips = 0ull, n_lanes = 0ull; // wave-uniform
    for (;;) {
        uint32_t base = 0;
        if (lane == 0u)
            base = atomicAdd(L.counters + WF_CNT_TICKET, (uint32_t)RT_PKT_CHUNK);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (base >= n_in)
            break;
        for (uint32_t q0 = base; q0 < base + RT_PKT_CHUNK && q0 < n_in; q0 += 64u) { // wave-uniform
            const uint32_t jq = q0 + lane;
            const bool have = jq < n_in;
            T.cur = T_DONE;
            if (have) {
                const WfRay ray = wf_load_ray(L.paths_in + wf_order_slot(L, jq));
                trav_init_stored<GB>(T, S.scene, ray.o, ray.d, ray.r, ray.fast);
                stk.reset();
            }
            for (;;) {
                trav_pop_wave<GB>(T, stk); // every lane that has to unwind does, until none is left in T_POP
                const uint32_t target = wave_min_u32(T.cur); // T_DONE is the largest value a lane can hold here
                if (target == T_DONE)
                    break;
                const bool mine = T.cur == target;
                const unsigned long long mm = __ballot(mine);
                if (mm == 0ull) // cannot happen (the minimum is some lane's value); never spin on a wrong reduction
                    break;
                ++n_trips; // how coherent the packets are: the host keeps or drops this kernel on lanes per trip
                n_lanes += (uint32_t)__popcll(mm);
                if ((target & RT_LEAF_FLAG) == 0u) {
                    // the record's address must stay a scalar: inside `if (mine)` the compiler knows T.cur == target and would
                    // otherwise address the node through the lane's own T.cur (a vector load per lane)
                    uint32_t node_index = target;
                    asm volatile("" : "+s"(node_index));
                    ConstF4 p = as_const_f4(nodes + node_index);
                    const F4v r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3];
                    if (mine)
                        trav_inner_apply<STATS, GB, false, REL>(T, stk, node_rec(r0, r1, r2, r3), EPS, st);
                } else { // a leaf: its triangles in index order, strict-less replacement (bvh.h:200-204,132)
                    const uint32_t cnt = RT_LEAF_CNT(target);
                    uint32_t k = target & RT_LEAF_BEGIN_MASK;
                    for (uint32_t i = 0;; ++i, ++k) {
                        ConstF4 p = as_const_f4(tris + k);
                        const F4v r0 = p[0], r1 = p[1], r2 = p[2];
                        const TriRec tri = tri_rec(r0, r1, r2);
                        if (mine) {
                            if (tri.flags & 2u)
                                st.node(); // one BVH::intersect_ray invocation on the leaf node
                            st.tri();
                            V3 xs;
                            if (REL ? tri_hit_folded(tri, T.d, EPS, xs) : tri_hit(tri, T.o, T.d, EPS, xs)) {
                                hit_take(T.best, k, xs.x, xs.y, xs.z);
                                T.t_loc = fminf(T.t_loc, xs.z);
                            }
                        }
                        if (cnt != 0u ? i + 1u == cnt : (tri.flags & 1u) != 0u)
                            break;
                    }
                    if (mine)
                        T.cur = T_POP;
                }
            }
            if (have)
                wf_store_hit(L.hits + jq, T.best);
        }
    }
    census_flush(L.packet_census, n_trips, n_lanes);
    st.flush(L.stats);
}

// The camera-relative copy of the binary tree's records for wf_extend_packet<.., REL>: what a lane computes from a record and the ray ORIGIN
// alone, computed once per (camera position, tree) instead of once per lane and trip. Same layouts, same indices:
//   node      the four corners become lmin - o, lmax - o, rmin - o, rmax - o (two_box's subtractions); child references unchanged
//   triangle  a becomes y = o - a (tri_rel_y), DevTri::pad (unused by the binary tree's kernels) the bits of nz = dot(v, crs(u, y)) (tri_rel_nz);
//             v, u, prim, flags unchanged
// Every value is the chain of single-rounding operations the lanes run on the same operands (-ffp-contract=off), hence the same bits.
// Grid-stride over 16-byte pieces would split a record's arithmetic; one lane per record, four / three 16-byte loads and stores each.
__global__ __launch_bounds__(256) void wf_camera_relative(const DevNode *nodes, uint32_t n_nodes, const DevTri *tris, uint32_t n_tris, V3 o, DevNode *rel_nodes, DevTri *rel_tris) {
    const uint32_t n = n_nodes + n_tris;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (i < n_nodes) {
            const float4 *p = reinterpret_cast<const float4 *>(nodes + i);
            const float4 r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3];
            const NodeRec r = node_rec(r0, r1, r2, r3);
            const V3 a = r.lmin - o, b = r.lmax - o, c = r.rmn - o, d = r.rmx - o;
            float4 *q = reinterpret_cast<float4 *>(rel_nodes + i);
            q[0] = make_float4(a.x, a.y, a.z, b.x);
            q[1] = make_float4(b.y, b.z, c.x, c.y);
            q[2] = make_float4(c.z, d.x, d.y, d.z);
            q[3] = r3;
        } else {
            const uint32_t k = i - n_nodes;
            const float4 *p = reinterpret_cast<const float4 *>(tris + k);
            const float4 r0 = p[0], r1 = p[1], r2 = p[2];
            const TriRec t = tri_rec(r0, r1, r2);
            const V3 y = tri_rel_y(t.a, o);
            const float nz = tri_rel_nz(t.v, t.u, y);
            float4 *q = reinterpret_cast<float4 *>(rel_tris + k);
            q[0] = make_float4(y.x, y.y, y.z, r0.w);
            q[1] = r1;
            q[2] = make_float4(r2.x, r2.y, r2.z, nz);
        }
    }
}

// ------------------------------------------------------------------------------------------------ extend: analytic primitives
// Scenes of the scene-txt front end may hold analytic primitives (ELLIPSOID / PLANE, include/rt_primspec.h) next to their
// triangles. They have no BVH (a plane is unbounded; BASELINE config 2 is "intersect kernel only, no BVH"): every queued
// ray tests all of them in index order and keeps the nearer of (BVH hit, primitive hit), strict-less as bvh.h:132.
// One lane per ray, records coalesced; launched only when the scene has such primitives.
__global__ __launch_bounds__(256) void wf_extend_prims(const DevScene S, const WfLaunch L) {
    const uint32_t n_in = L.counters[WF_CNT_IN];
    for (uint32_t jq = blockIdx.x * blockDim.x + threadIdx.x; jq < n_in; jq += gridDim.x * blockDim.x) {
        const WfHead ray = wf_load_head(L.paths_in + wf_order_slot(L, jq));
        Hit h = wf_load_hit(L.hits + jq);
        const uint32_t k0 = h.k;
        prims_closest(S, ray.o, ray.d, h);
        if (h.k != k0)
            wf_store_hit(L.hits + jq, h);
    }
}

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

// ------------------------------------------------------------------------------------------------ shade
// LIGHTS_LDS: the light BVH (inner nodes, triangles, aux) is small enough (DevBvh::lds_inner) to be staged in LDS once per
// block; bvh_mix_dist's sample and pdf then read it there: a dozen dependent L1 round trips per hit become LDS reads.
template <bool STATS, bool LIGHTS_LDS, int ENV> __global__ __launch_bounds__(256, RT_SHADE_WAVES_PER_SIMD) void wf_shade(const DevScene S, const WfLaunch L) {
    __shared__ float s_lin[256];
    __shared__ float s_gam[256];
    __shared__ uint32_t s_stack[STACK_LDS_DWORDS(RT_SHADE_LDS_DEPTH, 3)];
    __shared__ float4 s_lights[LIGHTS_LDS ? RT_SHADE_LIGHTS_F4 : 1];
    __shared__ uint2 s_perm[4][256]; // per wave: (queue position, queue slot) of its 256 positions, sorted by sampler class
    LightTabs LT = light_tabs_global(S);
    if (LIGHTS_LDS) {
        const uint32_t n_node_f4 = 4u * (S.lights.lds_inner - 1u), n_tri_f4 = 3u * S.lights.n_tris;
        for (uint32_t i = threadIdx.x; i < n_node_f4; i += blockDim.x)
            s_lights[i] = LT.nodes[i];
        for (uint32_t i = threadIdx.x; i < n_tri_f4; i += blockDim.x)
            s_lights[n_node_f4 + i] = LT.tris[i];
        for (uint32_t i = threadIdx.x; i < S.lights.n_tris; i += blockDim.x)
            s_lights[n_node_f4 + n_tri_f4 + i] = LT.aux[i];
        LT = LightTabs{s_lights, s_lights + n_node_f4, s_lights + n_node_f4 + n_tri_f4};
    }
    s_lin[threadIdx.x] = S.lut_linear[threadIdx.x];
    s_gam[threadIdx.x] = S.lut_gamma[threadIdx.x];
    __syncthreads();
    LaneStats<STATS> st;
    RT_DECLARE_STACK(stk, RT_SHADE_LDS_DEPTH, s_stack);
    const bool has_lights = S.lights.n_tris != 0; // raytracer.h:449-453
    const uint32_t n_in = L.counters[WF_CNT_IN];
    const uint32_t n_slots = (n_in + 63u) >> 6; // wave slots of this launch: positions 64w .. 64w+63
    // one shade() level for the hit at queue position jq (the ray in queue slot j), as the lanes of one wave; `wave_slot` is the wave slot
    // (64 positions) this trip stands for: survivors go to the sub-queue of that slot (rt_device_types.h, WF_STRIPES)
    auto shade_wave = [&](const uint32_t jq, const uint32_t j, const uint32_t wave_slot) {
        const bool active = jq < n_in;
        bool survive = false;
        WfPacked next;
        uint32_t next_key = 0u; // the ray-order key of `next`, made only when the next bounce may be sorted (WfLaunch::emit_keys)
        if (active) {
            const Hit h = wf_load_hit(L.hits + jq); // first: the attributes and texel addresses hang on the hit alone, and loads return in order
            const WfHead in = wf_load_head(L.paths_in + j); // its class bits chose this lane (below); nothing here reads them
            Rng<RT_RNG_DEVICE> rng = wf_load_rng(L.paths_in + j);
            const uint32_t path = in.id;
            uint32_t depth_left = in.depth_left, nb = in.nb;
            if (h.k != RT_NONE)
                depth_left -= 1; // shade(..., max_depth - 1)
            const ShadeResult sr = shade_hit<Rng<RT_RNG_DEVICE>, STATS, ENV>(S, LT, h, in.o, in.d, rng, has_lights, stk, s_lin, s_gam, st);
            bool terminal = sr.terminal;
            V3 term = sr.term;
            if (sr.push) // emission + trace_ray(...) * scl (raytracer.h:588-590), folded when the path ends
                wf_store_fold(L, nb++, path, sr.emission, sr.scl);
            if (!terminal && depth_left == 0) { // trace_ray(..., 0) returns (0,0,0) without casting (:596-598)
                terminal = true;
                term = mk(0, 0, 0);
            }
            if (terminal) {
                // The pending shade() frames are folded by wf_fold after the last bounce, not here: at any bounce only about a
                // quarter of a wave's paths end, each with its own number of frames, so the unwind ran at 16 of 64 lanes behind
                // dependent loads (14 % of this kernel's cycles). Leave the innermost value and the frame count.
                L.sample_out[path] = RtF4{term.x, term.y, term.z, __uint_as_float(nb)};
                st.sample();
            } else {
                survive = true;
                st.cast();
                next = wf_pack(sr.nro, sr.nrd, path, next_shade_class<ENV == ENV_FLOAT_DIST>(rng, has_lights), depth_left, nb, rng.g);
                if (L.emit_keys)
                    next_key = rt_ray_order_key(sr.nro.x, sr.nro.y, sr.nro.z, sr.nrd.x, sr.nrd.y, sr.nrd.z, S.bounds_lo, S.bounds_inv);
            }
        }
        // compact the survivors of this wave into the next queue: ballot + prefix sum, one atomic per wave, on the counter of
        // the sub-queue this wave slot belongs to (rt_device_types.h, WF_STRIPES)
        const unsigned long long m = __ballot(survive);
        if (m != 0ull) {
            const uint32_t rank = lane_rank(m);
            uint32_t obase = 0;
            const int leader = __ffsll((long long)m) - 1;
            const uint32_t stripe = /* the wave's own slot: a sub-queue holds what ITS slots can emit */ (uint32_t)__builtin_amdgcn_readfirstlane((int)wave_slot) % WF_STRIPES;
            if ((int)(threadIdx.x & 63u) == leader)
                obase = wf_stripe_base(stripe, n_slots) + atomicAdd(L.stripes + stripe * WF_STRIPE_WORDS, (uint32_t)__popcll(m));
            obase = __shfl(obase, leader);
            if (survive) {
                const uint32_t p = obase + rank;
                wf_store_path(L.paths_out + p, next);
                if (L.emit_keys) { // the sort's input, at the ray's physical slot: nobody reads the record again to make it
                    L.sort_keys[0][p] = next_key;
                    L.sort_vals[0][p] = wf_word(p, wf_word_class(__float_as_uint(next.p1.z))); // the class of the path word rides along above the slot (WfLaunch::order)
                }
            }
        }
    };
    // Which of shade()'s three samplers a hit runs is decided by its path's next draws alone (alpha coin, technique coin, mix pick:
    // raytracer.h:559,565,386): whoever wrote the path record left that class in the top bits of its path word, and the ray-order pass carried it along
    // in the top bits of `order`. A WAVE takes 256 queue positions at a time and hands them to its lanes sorted by class (a counting sort
    // over indices through the wave's own LDS window, before anything else is loaded, no block barrier): of its four trips one or two run
    // a single sampler and the others two instead of all three, and the rays aimed at a light walk the light BVH of bvh_mix_dist::pdf
    // side by side. Every wave still gets every class, so the waves of a block stay balanced. Which lane shades a hit changes no result.
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    // A queue too short to give every wave of the grid such a window is shaded 64 positions at a time (more waves, no reordering), and so
    // is one no sort ran over (primary rays; RT_SORT_OFF; the wide tree of a cache-resident scene): fetching the class from the records
    // ahead of the shading costs that kernel 6 % (measured, profiles/r04_variants.txt item 11); in the sort's payload it is free.
    const uint32_t win = (L.order_classed && n_in >= gridDim.x * 1024u) ? 256u : 64u;
    for (uint32_t wbase = (blockIdx.x * 4u + wv) * win; wbase < n_in; wbase += gridDim.x * 4u * win) { // wave-uniform
        uint32_t slot_of[4], cls[4], before[3] = {0u, 0u, 0u}, within[4];
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            const uint32_t jq = wbase + 64u * q + lane;
            slot_of[q] = jq, cls[q] = 3u; // class 3: the positions behind the queue's (or the window's) end
            if (64u * q < win && jq < n_in) {
                const uint32_t v = wf_order_word(L, jq);
                slot_of[q] = wf_word_slot(v), cls[q] = wf_word_class(v);
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) { // position inside the class: the class's members in earlier quarters, then in lower lanes
            const unsigned long long b0 = __ballot(cls[q] == 0u), b1 = __ballot(cls[q] == 1u), b2 = __ballot(cls[q] == 2u);
            const unsigned long long mine = cls[q] == 0u ? b0 : cls[q] == 1u ? b1 : cls[q] == 2u ? b2 : ~(b0 | b1 | b2);
            const uint32_t seen = cls[q] == 0u ? before[0] : cls[q] == 1u ? before[1] : cls[q] == 2u ? before[2] : 64u * q - before[0] - before[1] - before[2];
            within[q] = seen + lane_rank(mine);
            before[0] += (uint32_t)__popcll(b0), before[1] += (uint32_t)__popcll(b1), before[2] += (uint32_t)__popcll(b2);
        }
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
            const uint32_t start = cls[q] == 0u ? 0u : cls[q] == 1u ? before[0] : cls[q] == 2u ? before[0] + before[1] : before[0] + before[1] + before[2];
            s_perm[wv][start + within[q]] = make_uint2(wbase + 64u * q + lane, slot_of[q]);
        }
        __builtin_amdgcn_wave_barrier(); // the wave's LDS operations complete in order: its reads below see the writes above
        const uint32_t n_here = n_in - wbase < win ? n_in - wbase : win;
        for (uint32_t sub = 0; 64u * sub < n_here; ++sub) {
            const uint2 pj = s_perm[wv][64u * sub + lane];
            shade_wave(pj.x, pj.y, (wbase >> 6) + sub);
        }
        __builtin_amdgcn_wave_barrier();
    }
    st.flush(L.stats);
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

// ------------------------------------------------------------------------------------------------ probe: rays in, hits out
// rt_cast_rays_ex: arbitrary rays go through the SAME closest-hit kernels the renderer launches. wf_from_rays writes them as
// queue records (what wf_first_stage / wf_shade write for their rays), wf_hits_out turns the hit records into the probe's output.
__global__ __launch_bounds__(256) void wf_from_rays(const WfLaunch L, const float *rays, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0)
        L.counters[WF_CNT_IN] = n;
    if (i >= n)
        return;
    // one cast, no class, no frames, no RNG stream: nothing shades these rays
    wf_store_path(L.paths_in + i, wf_pack(ld3(rays + 6ull * i), ld3(rays + 6ull * i + 3), i, 0u, 1u, 0u, rt_xoshiro{{0u, 0u, 0u, 0u}}));
}
__global__ __launch_bounds__(256) void wf_hits_out(const DevScene S, const WfLaunch L, uint32_t n, uint32_t *prim_out, float *bct_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const Hit h = wf_load_hit(L.hits + i);
    const uint32_t k = h.k;
    if (k == RT_NONE) {
        prim_out[i] = RT_NONE;
        bct_out[3ull * i] = bct_out[3ull * i + 1] = bct_out[3ull * i + 2] = 0.0f;
    } else {
        prim_out[i] = (k & RT_PRIM_FLAG) ? S.n_triangles + (k & ~RT_PRIM_FLAG) : S.scene.tris[k].prim;
        bct_out[3ull * i] = h.b;
        bct_out[3ull * i + 1] = h.c;
        bct_out[3ull * i + 2] = h.t;
    }
}

} // namespace

namespace rt {

// One pass of the pipeline, fully stream-ordered (no host synchronisation): generate, ray_depth x (extend, shade,
// advance), resolve. `L.paths_in/paths_out` are swapped locally per bounce.
// every launch is checked: a failed launch (bad configuration, lost device) must not turn into a silently wrong image
#define WF_LAUNCH(...)                                  \
    do {                                                \
        if (hipError_t le_ = RT_LAUNCH_CHECKED(__VA_ARGS__); le_ != hipSuccess) \
            return le_;                                 \
    } while (0)

// positions the sub-queue regions written by a wf_shade over at most `bound` rays can span: whole wave slots (rt_device_types.h, WF_STRIPES)
static size_t wf_key_span(uint32_t bound) { return ((size_t)bound + 63u) / 64u * 64u; }

// the closest-hit kernel of one bounce: packets for coherent primary rays or the per-lane persistent kernel, each in the
// reference's traversal order (near-local pruning, the parity mode) or with global-best pruning (L.global_best, production)
static hipError_t launch_extend(const DevScene &S, const WfLaunch &L, bool packet, bool stats, int ext_blocks, hipStream_t stream) {
    if (S.scene.wide) // production build (RT_BUILD_WIDE): every bounce walks the 8-wide tree (rt_wide.hip)
        return launch_extend_wide(S, L, packet, stats, ext_blocks, stream);
    return with_bools([&](auto P, auto ST, auto G, auto R) {
        if constexpr (P)
            return RT_LAUNCH_CHECKED((wf_extend_packet<ST, G, R>), dim3(ext_blocks), dim3(256), 0, stream, S, L);
        else
            return RT_LAUNCH_CHECKED((wf_extend<ST, G>), dim3(ext_blocks), dim3(256), 0, stream, S, L);
    }, packet, stats, L.global_best != 0u, packet && L.rel_nodes != nullptr && L.rel_tris != nullptr);
}

hipError_t launch_camera_relative(const DevBvh &bvh, uint32_t n_nodes, const float *o, DevNode *rel_nodes, DevTri *rel_tris, int num_cus, hipStream_t stream) {
    const uint32_t n = n_nodes + bvh.n_tris;
    const uint32_t blocks = std::min<uint32_t>((n + 255u) / 256u, (uint32_t)num_cus * 16u);
    return RT_LAUNCH_CHECKED(wf_camera_relative, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, stream, bvh.nodes, n_nodes, bvh.tris, bvh.n_tris, V3{o[0], o[1], o[2]}, rel_nodes, rel_tris);
}

// ---- closest-hit probe through the production kernels (rt_cast_rays_ex): rays -> queue -> wf_extend / wf_extend_packet -> hits
hipError_t launch_wavefront_cast(const DevScene &S, WfLaunch L, const float *rays, uint32_t n, bool packet, bool stats, uint32_t *prim, float *bct,
                                 hipStream_t stream) {
    const dim3 block(256);
    hipError_t e = hipMemsetAsync(L.counters, 0, sizeof(uint32_t) * WF_CNT_WORDS, stream);
    if (e != hipSuccess)
        return e;
    L.n_paths = n;
    L.order = nullptr, L.order_classed = 0u;
    L.packet_census = nullptr;
    L.rel_nodes = nullptr, L.rel_tris = nullptr; // a caller's rays: any origin
    const int blocks = (int)((n + 255u) / 256u);
    WF_LAUNCH(wf_from_rays, dim3(blocks), block, 0, stream, L, rays, n);
    if ((e = launch_extend(S, L, packet, stats, (int)(L.stack_stride / 256u), stream)) != hipSuccess)
        return e;
    if (S.n_prims)
        WF_LAUNCH(wf_extend_prims, dim3(blocks), block, 0, stream, S, L);
    WF_LAUNCH(wf_hits_out, dim3(blocks), block, 0, stream, S, L, n, prim, bct);
    return hipSuccess;
}

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
    if (kind.source() == WfPassKind::LIST) { // the feature sums, the id tables and the group sums go before the sums: they read the entry's base count from the list
        const WfAccum &A = kind.entries();
        const WfLayers keep = kind.layers();
        const int res_blocks = (int)((A.n_entries + 255u) / 256u);
        if (keep.features)
            WF_LAUNCH(wf_resolve_features, dim3(res_blocks > 0 ? res_blocks : 1), block, 0, stream, A, *keep.features);
        if (keep.ids)
            WF_LAUNCH(wf_resolve_ids, dim3(res_blocks > 0 ? res_blocks : 1), block, 0, stream, A, *keep.ids);
        if (keep.groups)
            WF_LAUNCH(wf_resolve_groups, dim3(res_blocks > 0 ? res_blocks : 1), block, 0, stream, A, *keep.groups, L.n_paths);
        WF_LAUNCH(wf_resolve_list, dim3(res_blocks > 0 ? res_blocks : 1), block, 0, stream, L, A);
    } else if (kind.source() == WfPassKind::BAKE) { // the fold the bake's kind asks for, one lane per (point, k)
        const WfBake &B = kind.bake_points();
        const uint64_t lanes = (uint64_t)L.pass_pixels * (B.kind == RT_BAKE_SH9 ? 9u : 1u);
        const uint32_t bake_blocks = (uint32_t)std::min<uint64_t>((lanes + 255u) / 256u, (uint64_t)num_cus * 64u);
        WF_LAUNCH(wf_resolve_bake, dim3(bake_blocks > 0 ? bake_blocks : 1), block, 0, stream, L, B, first, last);
    } else { // cameras, a caller's rays: the image, or the outputs as a one-row image
        const int res_blocks = (int)((L.pass_pixels + 255u) / 256u);
        WF_LAUNCH(wf_resolve, dim3(res_blocks > 0 ? res_blocks : 1), block, 0, stream, L, first, last);
    }
    return hipSuccess;
}

hipError_t launch_wavefront_pass(const DevScene &S, WfLaunch L, const WfPassKind &kind, const WfPassStep &step, bool stats, int num_cus, hipStream_t stream,
                                 EventPool *extend_events, unsigned long long *packet_census_out, const WfHostSync *host_sync) {
    const int gen_blocks = (int)((L.n_paths + 255u) / 256u < (uint32_t)num_cus * 16u ? (L.n_paths + 255u) / 256u : (uint32_t)num_cus * 16u);
    const dim3 block(256);
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
    if ((e = launch_first_stage(S, L, kind, stats, dim3(gen_blocks > 0 ? gen_blocks : 1), stream)) != hipSuccess)
        return e;
    const int ext_blocks = (int)(L.stack_stride / 256u); // rt_scene.cpp sizes the overflow workspace for exactly this grid
    const int shade_blocks = num_cus * RT_SHADE_BLOCKS_PER_CU;
    // Queue sizes reach the host one bounce LATE and without ever idling the device: after bounce b's wf_advance the size of
    // queue b + 1 is copied to pinned word b + 1 and an event is recorded; bounce b + 2 waits for THAT event — by then bounce
    // b + 1's kernels are queued behind it, so the device has a whole bounce of work while the host looks. The host needs the
    // size only as an upper bound (grid of the ray-order pass, length of the sort, "nothing left": stop): the kernels read the
    // exact size from device memory. (Round 2 synchronised the stream once per bounce: eight idle gaps per pass.)
    const WfHostSync *hs = L.sort_mode != 0u || (packet && packet_census_out) ? host_sync : nullptr;
    if (hs && (!hs->counts || !hs->events || hs->n_events < (int)L.ray_depth + 1))
        hs = nullptr;
    // the per-bounce size read-back (one host wait per bounce from bounce 2 on) is only worth its latency where a sort follows; an unsorted
    // pass (a small one, rt_scene.cpp; or RT_SORT_OFF) is queued in one go and only the packet census, if any, is waited for once
    const bool want_bound = hs && L.sort_mode != 0u;
    uint32_t bound = L.n_paths; // upper bound of the queue entering the bounce about to be launched
    bool census_pending = false; // the packet census of bounce 0 is on its way to the pinned words (event 0)
    for (uint32_t b = 0; b < L.ray_depth; ++b) {
        L.order = nullptr, L.order_classed = 0u; // primary rays: dense and coherent as generated
        if (b > 0) {
            if (census_pending && b == 2) { // bounce 0's census: its copy is two bounces behind the queue head by now
                if ((e = hipEventSynchronize(hs->events[0])) != hipSuccess)
                    return e;
                std::memcpy(packet_census_out, hs->counts + WF_HOST_CENSUS_WORD, 2 * sizeof(unsigned long long));
                census_pending = false;
            }
            if (want_bound && b >= 2) { // size of queue b - 1, an upper bound of queue b
                if ((e = hipEventSynchronize(hs->events[b - 1])) != hipSuccess)
                    return e;
                bound = hs->counts[b - 1];
                if (bound == 0)
                    break;
            }
            // bound >= 4096 here implies bound >= 4096 at the bounce before (queues only shrink; bounce 1's bound is bounce 0's): the wf_shade
            // that wrote this queue was told to emit keys (below), over a pad fill at least as long as this sort
            const bool sort = want_bound && bound >= 4096u;
            if (sort) { // over the PHYSICAL positions of the queue: the producer had at most `bound` rays = wf_key_span(bound) / 64 wave slots
                size_t tmp = L.sort_temp_bytes;
                hipError_t se = rocprim::radix_sort_pairs(L.sort_temp, tmp, L.sort_keys[0], L.sort_keys[1], L.sort_vals[0], L.sort_vals[1], wf_key_span(bound), 0u, RT_RAY_KEY_BITS, stream);
                if (se != hipSuccess)
                    return se;
            } else { // dense ray index -> slot of paths_in (wf_shade's sub-queue regions)
                const uint32_t kb = (bound + 255u) / 256u < (uint32_t)num_cus * 16u ? (bound + 255u) / 256u : (uint32_t)num_cus * 16u;
                WF_LAUNCH(wf_sort_keys, dim3(kb > 0 ? kb : 1), block, 0, stream, L);
            }
            L.order = L.sort_vals[1];
            L.order_classed = sort ? 1u : 0u;
        }
        // time the dominant kernel per launch (bench.py roofline): HIP events on the launch stream, taken from the scene's
        // pool (created once, reused by every render)
        hipEvent_t e0 = extend_events ? extend_events->next() : nullptr;
        hipEvent_t e1 = e0 ? extend_events->next() : nullptr;
        if (e0 && e1)
            (void)hipEventRecord(e0, stream);
        if (hipError_t xe = launch_extend(S, L, b == 0 && packet, stats, ext_blocks, stream); xe != hipSuccess)
            return xe;
        if (e0 && e1)
            (void)hipEventRecord(e1, stream);
        if (S.n_prims)
            WF_LAUNCH(wf_extend_prims, dim3(shade_blocks), block, 0, stream, S, L);
        if (b == 0 && keep.features) // a feature accumulator's pass: the primary rays' first hits are final here
            WF_LAUNCH(wf_features, dim3(shade_blocks), block, 0, stream, S, L, *keep.features);
        if (b == 0 && keep.ids) // ... and so are their ids
            WF_LAUNCH(wf_ids, dim3(shade_blocks), block, 0, stream, S, L, *keep.ids);
        if (keep.groups) // light groups: at every bounce, whose emission the frame or terminal value wf_shade makes of this hit is
            WF_LAUNCH(wf_group_tags, dim3(shade_blocks), block, 0, stream, S, L, *keep.groups);
        // Will the next bounce be sorted? Its own bound is not known yet (it arrives one bounce late) but cannot exceed this one, so: may it be.
        // Then this wf_shade writes the sort's input itself, key and slot at the physical slot of every ray it makes, and every slot it leaves
        // empty (the ends of the 64 sub-queue regions) must already hold a pad: RT_RAY_KEY_PAD in the compared bits, behind every real key
        // wherever it stands. The regions of at most `bound` input rays end at wf_key_span(bound). (A byte fill of the range at HBM rate, a
        // few tens of microseconds; the bounce's own sort has read sort_keys[0] by now: it is earlier in the stream.)
        L.emit_keys = want_bound && b + 1 < L.ray_depth && bound >= 4096u ? 1u : 0u;
        if (L.emit_keys && (e = hipMemsetAsync(L.sort_keys[0], 0xFF, sizeof(uint32_t) * wf_key_span(bound), stream)) != hipSuccess)
            return e;
        // ENV: the scene has an environment map (DevScene::bg_tex): the miss branch looks it up (scene.h:83-89); those instantiations read the
        // light tables from global memory (LIGHTS_LDS only saves latency), so a scene without one never pays for the lookup's registers
        // A float map (rt_set_environment, DevScene::env) takes the texture's place: ENV_FLOAT, or ENV_FLOAT_DIST when it has a distribution
        // and mix_dist samples it. A scene without one launches what it always launched.
        const bool fenv = S.env.texels != nullptr;
        const bool env = fenv ? S.env.marg != nullptr : S.bg_tex >= 0;
        const bool lights_lds = S.lights.lds_inner != 0u && !env && !fenv;
        e = with_bools([&](auto ST, auto LDS, auto FENV, auto ENV) {
            constexpr int KIND = FENV ? (ENV ? ENV_FLOAT_DIST : ENV_FLOAT) : (ENV ? ENV_TEX8 : ENV_NONE);
            if constexpr (LDS && KIND != ENV_NONE) // never chosen (above), never instantiated
                return hipErrorInvalidValue;
            else
                return RT_LAUNCH_CHECKED((wf_shade<ST, LDS, KIND>), dim3(shade_blocks), block, 0, stream, S, L);
        }, stats, lights_lds, fenv, env);
        if (e != hipSuccess)
            return e;
        WF_LAUNCH(wf_advance, dim3(1), dim3(64), 0, stream, L.counters, L.stripes);
        if (hs && b == 0 && packet && packet_census_out) { // the packet kernel's census -> pinned words; read at bounce 2, or behind the loop
            if ((e = hipMemcpyAsync(hs->counts + WF_HOST_CENSUS_WORD, L.packet_census, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream)) != hipSuccess)
                return e;
            if ((e = hipEventRecord(hs->events[0], stream)) != hipSuccess)
                return e;
            census_pending = true;
        }
        if (want_bound && b + 1 < L.ray_depth) { // size of queue b + 1 -> pinned word b + 1 (read by bounce b + 2)
            if ((e = hipMemcpyAsync(hs->counts + b + 1, L.counters + WF_CNT_IN, sizeof(uint32_t), hipMemcpyDeviceToHost, stream)) != hipSuccess)
                return e;
            if ((e = hipEventRecord(hs->events[b + 1], stream)) != hipSuccess)
                return e;
        }
        WfPath *t = L.paths_in;
        L.paths_in = L.paths_out;
        L.paths_out = t;
    }
    if (keep.groups) // before wf_fold, which overwrites the terminal values in sample_out
        WF_LAUNCH(wf_fold_groups, dim3(gen_blocks > 0 ? gen_blocks : 1), block, 0, stream, L, *keep.groups);
    WF_LAUNCH(wf_fold, dim3(gen_blocks > 0 ? gen_blocks : 1), block, 0, stream, L);
    if (census_pending) { // ray_depth <= 2 (no bounce 2 to read it at): wait for bounce 0 only; the rest of the pass is queued behind it
        if ((e = hipEventSynchronize(hs->events[0])) != hipSuccess)
            return e;
        std::memcpy(packet_census_out, hs->counts + WF_HOST_CENSUS_WORD, 2 * sizeof(unsigned long long));
    }
    return launch_last_stage(L, kind, step, num_cus, stream);
}

hipError_t launch_sensor_rays(const WfSensor *d_sensor, uint32_t width, uint32_t height, uint32_t first_pixel, uint32_t first_sample, uint32_t samples, uint32_t n,
                              void *d_rays_out, int num_cus, hipStream_t stream) {
    const uint32_t blocks = std::min<uint32_t>((n + 255u) / 256u, (uint32_t)num_cus * 16u);
    return RT_LAUNCH_CHECKED(wf_sensor_rays, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, stream, d_sensor, width, height, first_pixel, first_sample, samples, n,
                             static_cast<uint4 *>(d_rays_out));
}

hipError_t launch_bake_rays(const WfBake &B, uint32_t samples, uint32_t n, void *d_rays_out, int num_cus, hipStream_t stream) {
    const uint32_t blocks = std::min<uint32_t>((n + 255u) / 256u, (uint32_t)num_cus * 16u);
    return RT_LAUNCH_CHECKED(wf_bake_rays, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, stream, B, samples, n, static_cast<uint4 *>(d_rays_out));
}

size_t wavefront_sort_temp_bytes(size_t n) {
    size_t tmp = 0;
    uint32_t *k = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, tmp, k, k, k, k, n, 0u, 27u, (hipStream_t) nullptr);
    return tmp;
}

} // namespace rt
