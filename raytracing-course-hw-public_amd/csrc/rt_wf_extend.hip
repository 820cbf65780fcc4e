// rt_wf_extend.hip — closest hit over the binary tree for the wavefront pipeline (rt_wavefront.hip: the pipeline and its scheduler): wf_extend
// (persistent wavefronts, one ray per lane), wf_extend_packet (coherent primary rays, one record per trip; camera-relative records from
// wf_camera_relative), wf_extend_prims (analytic primitives), and the closest-hit probe that sends a caller's rays through the same kernels.
// Scenes built with RT_BUILD_WIDE walk the 8-wide tree instead (rt_wide.hip); launch_extend dispatches.
#include "rt_dev_queue.h"
#include "rt_dev_stack.h"
#include "rt_dev_trav.h"
#include "rt_kernels.h"
#include "rt_wf_policy.h"
#include "rt_wf_records.h"

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

// The compact records of a binary tree (DevNodeCompact) and the selector / valid bits in DevNode::sel, derived from the DevNode array once it
// is final: one lane per inner node runs compact_derive_node (rt_device_types.h: the rule, and why the lanes do not race).
__global__ __launch_bounds__(256) void wf_derive_compact(DevNode *nodes, uint32_t n_nodes, DevNodeCompact *compact) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += gridDim.x * blockDim.x)
        compact_derive_node(reinterpret_cast<uint32_t *>(nodes), n_nodes, i, reinterpret_cast<uint32_t *>(compact));
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

// the closest-hit kernel of one bounce: packets for coherent primary rays or the per-lane persistent kernel, each in the
// reference's traversal order (near-local pruning, the parity mode) or with global-best pruning (L.global_best, production)
hipError_t launch_extend(const DevScene &S, const WfLaunch &L, bool packet, bool stats, hipStream_t stream) {
    const int ext_blocks = (int)(L.stack_stride / 256u); // rt_scene.cpp sizes the overflow workspace for exactly this grid
    if (S.scene.wide) // production build (RT_BUILD_WIDE): every bounce walks the 8-wide tree (rt_wide.hip)
        return launch_extend_wide(S, L, packet, stats, ext_blocks, stream);
    return with_bools([&](auto P, auto ST, auto G, auto R) {
        if constexpr (P)
            return RT_LAUNCH_CHECKED((wf_extend_packet<ST, G, R>), dim3(ext_blocks), dim3(256), 0, stream, S, L);
        else
            return RT_LAUNCH_CHECKED((wf_extend<ST, G>), dim3(ext_blocks), dim3(256), 0, stream, S, L);
    }, packet, stats, L.global_best != 0u, packet && L.rel_nodes != nullptr && L.rel_tris != nullptr);
}

hipError_t launch_extend_prims(const DevScene &S, const WfLaunch &L, uint32_t blocks, hipStream_t stream) {
    return RT_LAUNCH_CHECKED(wf_extend_prims, dim3(blocks), dim3(256), 0, stream, S, L);
}

hipError_t launch_camera_relative(const DevBvh &bvh, uint32_t n_nodes, const float *o, DevNode *rel_nodes, DevTri *rel_tris, int num_cus, hipStream_t stream) {
    const uint32_t n = n_nodes + bvh.n_tris;
    return RT_LAUNCH_CHECKED(wf_camera_relative, dim3(wf_grid_stride(n, num_cus, 16u)), dim3(256), 0, stream, bvh.nodes, n_nodes, bvh.tris, bvh.n_tris, V3{o[0], o[1], o[2]}, rel_nodes, rel_tris);
}

hipError_t launch_derive_compact(DevNode *nodes, uint32_t n_nodes, DevNodeCompact *compact, int num_cus, hipStream_t stream) {
    if (n_nodes == 0u)
        return hipSuccess;
    if (hipError_t e = hipMemsetAsync(compact, 0, sizeof(DevNodeCompact) * (size_t)n_nodes, stream); e != hipSuccess)
        return e;
    return RT_LAUNCH_CHECKED(wf_derive_compact, dim3(wf_grid_stride(n_nodes, num_cus, 16u)), dim3(256), 0, stream, nodes, n_nodes, compact);
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
    const dim3 grid(wf_grid_items(n)); // n >= 1: rt_cast_rays_ex returns before it stages anything for no rays (rt_probe.cpp)
    WF_LAUNCH(wf_from_rays, grid, block, 0, stream, L, rays, n);
    if ((e = launch_extend(S, L, packet, stats, stream)) != hipSuccess)
        return e;
    if (S.n_prims && (e = launch_extend_prims(S, L, grid.x, stream)) != hipSuccess)
        return e;
    WF_LAUNCH(wf_hits_out, grid, block, 0, stream, S, L, n, prim, bct);
    return hipSuccess;
}

} // namespace rt
