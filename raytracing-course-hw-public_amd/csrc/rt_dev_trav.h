// rt_dev_trav.h — closest hit and light-pdf traversal of the binary BVH: exact slab / triangle tests, the node and triangle record views, the hit
// rule, the resumable traversal steps and pops, and the cooperative triangle batch. Reference citations are next to each function.
#pragma once
#include "../../include/rt_primspec.h"
#include "rt_dev_math.h"

namespace {

// ---------------------------------------------------------------------------------------------- primitives
// Exact quotient a/d from a precomputed r = RN(1/d): q0 = RN(a*r), one FMA residual e = a - d*q0 and one FMA correction
// q1 = RN(q0 + e*r) = RN(a/d). 3 VALU ops instead of the ~11-op IEEE division expansion (v_div_scale / v_rcp / ... /
// v_div_fixup). Why one correction suffices although q0 may be off by 1.5 ulp (Markstein's theorem wants a faithful
// q0): the value rounded last is Q + (Q - q0)*eps with |eps| <= 2^-24, i.e. within ~3*2^-24 ulp of Q = a/d, and a
// quotient of two 24-bit significands comes that close to a rounding boundary only for the finitely many pairs with
// |A*2^k - B*m| <= 16 — all 93 million of which tools/proofs/div_one_step.c enumerates and checks against IEEE division
// (run by tests/test_host_and_abi.py). The residual must be exactly representable and nothing may overflow/underflow;
// that is guaranteed per RAY and per SCENE, not per box:
//   * every direction component has |d_i| in [2^-40, 2^40]                                   (trav_init)
//   * every origin component and every box coordinate is 0 or has magnitude in [2^-37, 2^40] (trav_init, host)
// so a = box - o is 0 or a multiple of 2^-60 with |a| <= 2^41, hence q = 0 or 2^-100 <= |q| <= 2^81, all normal.
// Rays (or scenes) outside these bounds take the reference IEEE division instead.
DEV float div_exact_fast(float a, float d, float r) {
    const float q0 = a * r;
    const float e0 = __builtin_fmaf(-d, q0, a);
    return __builtin_fmaf(e0, r, q0);
}
constexpr float RANGE_LO = 9.094947017729282e-13f;  // 2^-40
constexpr float RANGE_HI = 1099511627776.0f;        // 2^40
constexpr float ORIGIN_LO = 7.275957614183426e-12f; // 2^-37
DEV bool coord_in_fast_range(float c) { // 0, or 2^-37 <= |c| <= 2^40 (false for NaN / inf)
    const float m = __builtin_fabsf(c);
    return (c == 0.0f) | ((m >= ORIGIN_LO) & (m <= RANGE_HI));
}

// intersect(ray, aabb, min_dst) bvh.h:137-152, reference form: IEEE division, std::min/max operand order kept by
// explicit selects, component reductions as std::max_element / std::min_element (first extremum, geometry.h:42-50).
// Both slab tests take the box corners RELATIVE to the ray origin, a1 = bmin - o and a2 = bmax - o: two_box makes them from an absolute
// record, or passes on what a camera-relative record holds (wf_camera_relative: each corner the same single IEEE subtraction, the same bits).
DEV bool box_hit_exact_rel(V3 a1, V3 a2, V3 d, float min_dst, float &dist) {
    V3 i1 = a1 / d;
    V3 i2 = a2 / d;
    V3 mn = {rmin(i1.x, i2.x), rmin(i1.y, i2.y), rmin(i1.z, i2.z)};
    V3 mx = {rmax(i1.x, i2.x), rmax(i1.y, i2.y), rmax(i1.z, i2.z)};
    float t_min = mn.x;
    if (t_min < mn.y)
        t_min = mn.y;
    if (t_min < mn.z)
        t_min = mn.z;
    float t_max = mx.x;
    if (mx.y < t_max)
        t_max = mx.y;
    if (mx.z < t_max)
        t_max = mx.z;
    if (t_min <= t_max && t_max >= min_dst) {
        dist = rmax(t_min, min_dst);
        return true;
    }
    return false;
}

// Same slab test on the fast path: the six quotients come from div_exact_fast and are the correctly rounded finite
// quotients (see above), so there is no NaN and no infinity among them and v_min/v_max agree with the reference's
// select forms up to the sign of a zero, which cannot reach the result: t_min/t_max are only compared, and
// max(t_min, min_dst) with min_dst = 1e-4 > 0 never returns a zero.
DEV bool box_hit_fast_rel(V3 a1, V3 a2, V3 d, V3 r, float min_dst, float &dist) {
    float q1x = div_exact_fast(a1.x, d.x, r.x), q1y = div_exact_fast(a1.y, d.y, r.y), q1z = div_exact_fast(a1.z, d.z, r.z);
    float q2x = div_exact_fast(a2.x, d.x, r.x), q2y = div_exact_fast(a2.y, d.y, r.y), q2z = div_exact_fast(a2.z, d.z, r.z);
    float t_min = fmaxf(fmaxf(fminf(q1x, q2x), fminf(q1y, q2y)), fminf(q1z, q2z));
    float t_max = fminf(fminf(fmaxf(q1x, q2x), fmaxf(q1y, q2y)), fmaxf(q1z, q2z));
    dist = fmaxf(t_min, min_dst);
    return (t_min <= t_max) & (t_max >= min_dst);
}

// The two BVH records as the kernels hold them: built ONCE from the record's 16-byte pieces, whichever way those were loaded (float4: a vector
// load per lane; F4v: one scalar load for the wave, rt_dev_math.h as_const_f4).
//   DevNode = lmin.xyz lmax.xyz rmin.xyz rmax.xyz left right sel -      DevTri = a.xyz v.xyz u.xyz prim flags index
struct NodeRec {
    V3 lmin, lmax, rmn, rmx;
    uint32_t left, right;
};
template <class P, class P3> DEV NodeRec node_rec(const P &r0, const P &r1, const P &r2, const P3 &r3) {
    return NodeRec{mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x), mk(r2.y, r2.z, r2.w), __float_as_uint(r3.x), __float_as_uint(r3.y)};
}
struct TriRec {
    V3 a, v, u;
    uint32_t flags, index; // flags: 1 = last triangle of its leaf, 2 = first; index: DevTri::pad, the DevTri / DevAttr index of a wide-blob record
};
template <class P> DEV TriRec tri_rec(const P &r0, const P &r1, const P &r2) {
    return TriRec{mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), mk(r1.z, r1.w, r2.x), __float_as_uint(r2.z), __float_as_uint(r2.w)};
}

// intersect_ray_triangle + intersect(ray, triangle, min_dst) bvh.h:36-65 (Cramer; xs = (b, c, t)).
// det(c1,c2,c3) = dot(c1, crs(c2,c3)) (geometry.h:26-29); crs(u, -d) is shared by two determinants.
// Division-free rejection filter. With D = |den| in [2^-60, 2^60] and sign-adjusted numerators n' = n * sign(den)
// (so the exact quotients are X = nx'/D, Y = ny'/D, Z = nz'/D) a triangle CERTAINLY fails the reference's test
//     xs.x >= 0 && xs.y >= 0 && xs.x + xs.y <= 1 && xs.z >= min_dst          (bvh.h:59-60, xs = RN(n/den))
// when  nx' < -2^-60  or  ny' < -2^-60           (X or Y < -2^-120: the rounded quotient is negative, not -0)
//   or  nx' + ny' > D * (1 + 2^-20)               (X + Y > 1 + 2^-20: beyond the three roundings, ~3 * 2^-24)
//   or  nz' < D * min_dst * (1 - 2^-20)           (Z < min_dst beyond the rounding of RN(Z))
// Anything else ("maybe") takes the reference's three IEEE divisions and its exact comparisons, so the filter only
// removes work, never changes an outcome. NaN/inf operands make every comparison false -> "maybe".
// tri_hit_rel is the test behind everything that does not depend on the ray direction: y = o - a and nz = dot(v, crs(u, y)) are given. tri_hit
// makes them from the record; the camera-relative records hold them (tri_rel_y / tri_rel_nz: the same operations on the same operands).
DEV bool tri_hit_rel(V3 av, V3 au, V3 y, float nz, V3 d, float min_dst, V3 &xs_out) {
    V3 at = -d;
    V3 c_ut = crs(au, at);
    float den = dot(av, c_ut);
    float nx = dot(y, c_ut), ny = dot(av, crs(y, at));
    const uint32_t sgn = __float_as_uint(den) & 0x80000000u;
    const float D = __builtin_fabsf(den);
    const float nxs = __uint_as_float(__float_as_uint(nx) ^ sgn), nys = __uint_as_float(__float_as_uint(ny) ^ sgn),
                nzs = __uint_as_float(__float_as_uint(nz) ^ sgn);
    const bool d_ok = (D >= 8.673617379884035e-19f) & (D <= 1.152921504606847e18f); // 2^-60 .. 2^60
    const bool miss = (nxs < -8.673617379884035e-19f) | (nys < -8.673617379884035e-19f) | (nxs + nys > D * 1.00000095367431640625f) |
                      (nzs < D * (min_dst * 0.99999904632568359375f));
    if (d_ok & miss)
        return false;
    V3 xs = V3{nx, ny, nz} / den;
    if (xs.x >= 0 && xs.y >= 0 && xs.x + xs.y <= 1 && xs.z >= min_dst) {
        xs_out = xs;
        return true;
    }
    return false;
}
DEV V3 tri_rel_y(V3 a, V3 o) { return o - a; }
DEV float tri_rel_nz(V3 av, V3 au, V3 y) { return dot(av, crs(au, y)); }
DEV bool tri_hit(const TriRec &tri, V3 o, V3 d, float min_dst, V3 &xs_out) {
    const V3 y = tri_rel_y(tri.a, o);
    return tri_hit_rel(tri.v, tri.u, y, tri_rel_nz(tri.v, tri.u, y), d, min_dst, xs_out);
}
// a camera-relative triangle record (wf_camera_relative): y in the place of a, the bits of nz in the place of DevTri::pad
DEV bool tri_hit_folded(const TriRec &tri, V3 d, float min_dst, V3 &xs_out) { return tri_hit_rel(tri.v, tri.u, tri.a, __uint_as_float(tri.index), d, min_dst, xs_out); }

struct Hit {
    uint32_t k; // DevTri index (BVH order) or RT_NONE
    float b, c, t;
};
// update_intersection (bvh.h:132): a candidate replaces the best hit iff there is none yet or the existing t is STRICTLY greater, so of two
// hits with equal t the one found first stays. (A traversal whose best.t starts at +inf satisfies the first clause through the second.)
DEV void hit_take(Hit &best, uint32_t k, float b, float c, float t) {
    if (best.k == RT_NONE || best.t > t) {
        best.k = k;
        best.b = b;
        best.c = c;
        best.t = t;
    }
}

// Analytic primitives (scene-txt ELLIPSOID / PLANE, include/rt_primspec.h): tested by brute force AFTER the BVH, in index
// order, with the same strict-less replacement as update_intersection (bvh.h:132) — the CPU oracle does exactly this.
DEV rt_primitive_desc load_prim(const rt_primitive_desc *prims, uint32_t i) {
    rt_primitive_desc p;
    const uint4 *src = reinterpret_cast<const uint4 *>(prims + i); // 48-byte records, 16-byte aligned
    uint4 *dst = reinterpret_cast<uint4 *>(&p);
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
    return p;
}
DEV void prims_closest(const DevScene &S, V3 o, V3 d, Hit &best) {
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    for (uint32_t i = 0; i < S.n_prims; ++i) {
        const rt_primitive_desc p = load_prim(S.prims, i);
        float t, n[3];
        if (rt_prim_intersect(&p, oo, dd, 1e-4f /* EPS, config.h:15 */, &t, n))
            hit_take(best, RT_PRIM_FLAG | i, 0.0f, 0.0f, t);
    }
}

// ---------------------------------------------------------------------------------------------- closest hit
// BVH::intersect_ray (bvh.h:170-180, 195-235) as a resumable per-lane state machine: one call of trav_step visits
// ONE record — an inner node (both child boxes, 64 B) or one leaf triangle (48 B) — so every lane of the wavefront
// issues exactly one gather per step whatever it is doing, and a lane can be parked between steps while others shade.
//   frame = {far child ref, far entry distance d_far, local best of the ENCLOSING subtree at push time}
//   t_loc = local best t of the subtree being traversed (NaN = no hit yet; fminf ignores NaN operands).
// On pop the far sibling is visited iff the near subtree found nothing or found t > d_far (bvh.h:221): the
// reference prunes against the near subtree's local best only. The global best uses the strict "replace iff existing
// t > new t" rule (bvh.h:132) in DFS order, which equals the nested update_intersection calls.
constexpr uint32_t T_DONE = 0xFFFFFFFEu, T_POP = 0xFFFFFFFDu;
struct Trav {
    V3 o, d, r; // r = 1/d (IEEE) for div_exact_fast
    uint32_t cur;
    int sp;
    float t_loc;
    Hit best;
    bool fast; // div_exact_fast is valid for this ray (see its comment)
    // newest frame (stack position sp-1) cached in registers: a pop followed by a node visit never waits for LDS
    uint32_t top_ref;
    float top_d, top_loc;
};
// div_exact_fast's preconditions: the per-ray half (stored with a queued ray, WfPath::fast) and, with the per-scene half the host checked
// (DevBvh::fast_ok), the whole
DEV bool ray_fast_ok_ray(V3 o, V3 d) {
    const float lo = fminf(fminf(__builtin_fabsf(d.x), __builtin_fabsf(d.y)), __builtin_fabsf(d.z));
    const float hi = fmaxf(fmaxf(__builtin_fabsf(d.x), __builtin_fabsf(d.y)), __builtin_fabsf(d.z));
    // one straight-line predicate (bitwise on purpose: no short-circuit branches); the casts say so to -Wall
    return (d.x == d.x) & (d.y == d.y) & (d.z == d.z) & (lo >= RANGE_LO) & (hi <= RANGE_HI) & (int)coord_in_fast_range(o.x) & (int)coord_in_fast_range(o.y) &
           (int)coord_in_fast_range(o.z);
}
DEV bool ray_fast_ok(const DevBvh &bvh, V3 o, V3 d) {
    const bool ray_ok = ray_fast_ok_ray(o, d);
    return ray_ok & (bvh.fast_ok != 0u);
}
// GB (production traversal, RT_FLAG_GLOBAL_BEST): T.t_loc is the GLOBAL best t so far (+inf before the first hit) and every
// box is culled against it: a child is visited iff !(best.t <= its entry distance). The reference prunes a far child only
// against the near subtree's local best (bvh.h:216-223), so the global rule visits a SUBSET of the reference's nodes and
// returns the same hit unless a triangle's t rounds below its own box's entry distance — measured per scene by
// tests/test_gpu_production.py. Frames shrink to {ref, d_far}: no saved local best.
template <bool GB = false> DEV void trav_init_stored(Trav &T, const DevBvh &bvh, V3 o, V3 d, V3 r, bool ray_ok) {
    T.o = o;
    T.d = d;
    T.r = r;
    T.fast = ray_ok & (bvh.fast_ok != 0u);
    T.cur = (bvh.root == RT_NONE || bvh.n_tris == 0) ? T_DONE : bvh.root;
    T.sp = 0;
    T.t_loc = GB ? RT_INF : RT_NAN;
    if constexpr (GB)
        T.top_loc = 0.0f; // unused by the global-best frames
    T.best = Hit{RT_NONE, 0.f, 0.f, 0.f};
}
// ... and from a ray made on the spot (megakernel, probes): 1 / d by IEEE division
DEV void trav_init(Trav &T, const DevBvh &bvh, V3 o, V3 d) { trav_init_stored<false>(T, bvh, o, d, mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z), ray_fast_ok_ray(o, d)); }
// a lane without a ray: nothing to visit, every field defined
template <bool GB = false> DEV Trav trav_idle() {
    Trav T;
    T.o = T.d = T.r = mk(0.f, 0.f, 0.f);
    T.cur = T_DONE;
    T.sp = 0;
    T.t_loc = GB ? RT_INF : RT_NAN;
    T.best = Hit{RT_NONE, 0.f, 0.f, 0.f};
    T.fast = false;
    T.top_ref = 0u;
    T.top_d = T.top_loc = 0.f;
    return T;
}

// Unwind deferred siblings after a leaf or a double miss: the far child of the newest frame is visited iff the near
// subtree found nothing or found t > d_far (bvh.h:221); either way the near result is merged into the enclosing
// subtree's local best. Ends in T_DONE when the stack is empty.
template <class STK> DEV void trav_pop(Trav &T, STK &stk) {
    while (T.cur == T_POP) {
        if (T.sp == 0) {
            T.cur = T_DONE;
            break;
        }
        --T.sp;
        const uint32_t ref = T.top_ref;
        const float dfar = T.top_d, saved = T.top_loc;
        if (T.sp > 0)
            stk.pop(T.sp - 1, T.top_ref, T.top_d, T.top_loc); // refill the register copy; consumed at the next pop
        const float t_near = T.t_loc;
        T.t_loc = fminf(saved, t_near);
        if (!(t_near <= dfar)) // !has || t_near > d_far (bvh.h:221)
            T.cur = ref;
    }
}

// The two child boxes of a node against one ray: hit flags and entry distances. Exact-quotient division where the ray allows it (`fast`),
// the reference's IEEE division otherwise; KNOWN_FAST: the caller has established `fast` for every lane it sends here, no branch is compiled.
struct TwoBox {
    bool hl, hr;
    float dl, dr;
};
// REL: the record's four corners are relative to the ray origin already (a camera-relative record): `o` is not read.
template <bool KNOWN_FAST = false, bool REL = false> DEV TwoBox two_box(const NodeRec &n, V3 o, V3 d, V3 r, bool fast, float min_dst) {
    const V3 l1 = REL ? n.lmin : n.lmin - o, l2 = REL ? n.lmax : n.lmax - o, r1 = REL ? n.rmn : n.rmn - o, r2 = REL ? n.rmx : n.rmx - o;
    TwoBox b;
    if (KNOWN_FAST || fast) {
        b.hl = box_hit_fast_rel(l1, l2, d, r, min_dst, b.dl);
        b.hr = box_hit_fast_rel(r1, r2, d, r, min_dst, b.dr);
    } else { // rare ray: a direction/origin component is 0-adjacent, huge or NaN -> reference arithmetic
        b.hl = box_hit_exact_rel(l1, l2, d, min_dst, b.dl);
        b.hr = box_hit_exact_rel(r1, r2, d, min_dst, b.dr);
    }
    return b;
}
// THE inner-node step, on a record the caller holds: test both child boxes, order them near / far, defer the far one. Written so that a wave
// runs one straight-line sequence (selects instead of per-lane branches: no exec-mask nesting and no register copies at control-flow joins).
// Leaves T.cur == T_POP when the lane has to unwind; the caller chooses how (trav_pop: per-lane loop; trav_pop_once / trav_pop_wave: all
// lanes of the wave together).
template <bool STATS, bool GB = false, bool KNOWN_FAST = false, bool REL = false, class STK>
DEV void trav_inner_apply(Trav &T, STK &stk, const NodeRec &n, float min_dst, LaneStats<STATS> &st) {
    st.node();
    st.box(2);
    const TwoBox bx = two_box<KNOWN_FAST, REL>(n, T.o, T.d, T.r, T.fast, min_dst);
    bool hl = bx.hl, hr = bx.hr;
    const float dl = bx.dl, dr = bx.dr;
    if constexpr (GB) { // cull against the global best
        hl = hl && dl < T.t_loc;
        hr = hr && dr < T.t_loc;
    }
    const bool both = hl & hr;
    const bool swap = dl > dr; // bvh.h:216 (ties keep left first)
    if (both & (T.sp > 0))
        stk.push(T.sp - 1, T.top_ref, T.top_d, T.top_loc); // spill the previous top
    T.top_ref = both ? (swap ? n.left : n.right) : T.top_ref;
    T.top_d = both ? (swap ? dl : dr) : T.top_d;
    if constexpr (!GB) {
        T.top_loc = both ? T.t_loc : T.top_loc;
        T.t_loc = both ? RT_NAN : T.t_loc;
    }
    T.sp += both ? 1 : 0;
    T.cur = both ? (swap ? n.right : n.left) : (hl ? n.left : (hr ? n.right : T_POP));
}
// One record per call, whatever the lane stands on: an inner node (load, then apply) or one triangle of a big leaf.
template <bool STATS, bool GB = false, class STK> DEV void trav_step_core(Trav &T, const DevBvh &bvh, STK &stk, float min_dst, LaneStats<STATS> &st) {
    const bool leaf = (T.cur & RT_LEAF_FLAG) != 0;
    const float4 *p = leaf ? reinterpret_cast<const float4 *>(bvh.tris + (T.cur & RT_LEAF_BEGIN_MASK)) : reinterpret_cast<const float4 *>(bvh.nodes + T.cur);
    const float4 r0 = p[0], r1 = p[1], r2 = p[2];
    if (!leaf) {
        trav_inner_apply<STATS, GB>(T, stk, node_rec(r0, r1, r2, p[3]), min_dst, st);
    } else {
        const TriRec tri = tri_rec(r0, r1, r2);
        if (tri.flags & 2u)
            st.node(); // first triangle of its leaf: one BVH::intersect_ray invocation on the leaf node
        st.tri();
        V3 xs;
        if (tri_hit(tri, T.o, T.d, min_dst, xs)) {
            hit_take(T.best, T.cur & RT_LEAF_BEGIN_MASK, xs.x, xs.y, xs.z);
            T.t_loc = fminf(T.t_loc, xs.z);
        }
        T.cur = (tri.flags & 1u) ? T_POP : T.cur + 1;
    }
}
template <bool STATS, class STK> DEV void trav_step(Trav &T, const DevBvh &bvh, STK &stk, float min_dst, LaneStats<STATS> &st) {
    trav_step_core<STATS, false>(T, bvh, stk, min_dst, st);
    trav_pop(T, stk);
}
// A compact record (DevNodeCompact, rt_device_types.h) expanded with the node's own box {bmin, bmax} and its six selector bits: the record
// node_rec makes of the node's DevNode, bit for bit, when the parent says `valid` (wf_derive_compact compared all twelve planes).
DEV NodeRec node_rec_compact(const float4 &c0, const float4 &c1, V3 bmin, V3 bmax, uint32_t sel) {
    const bool s0 = sel & 1u, s1 = sel & 2u, s2 = sel & 4u, s3 = sel & 8u, s4 = sel & 16u, s5 = sel & 32u;
    return NodeRec{mk(s0 ? c0.x : bmin.x, s1 ? c0.y : bmin.y, s2 ? c0.z : bmin.z), mk(s3 ? c0.w : bmax.x, s4 ? c1.x : bmax.y, s5 ? c1.y : bmax.z),
                   mk(s0 ? bmin.x : c0.x, s1 ? bmin.y : c0.y, s2 ? bmin.z : c0.z), mk(s3 ? bmax.x : c0.w, s4 ? bmax.y : c1.x, s5 ? bmax.z : c1.y),
                   __float_as_uint(c1.z), __float_as_uint(c1.w)};
}
// The node step for lanes the caller knows to be on an inner node with T.fast (wf_extend's hot loop): load, then apply without the guard.
// Two visits per trip where the tree has compact records (DevBvh::compact): a lane that steps straight into an inner child (the near child
// of a double hit or the only child hit; not a pop) holds that child's box in the record it has just read, and visits the child at once
// from its 32-byte compact record: 2 vector-L1 accesses instead of 4. Nothing of the box outlives the call: the next trip starts on T.cur
// with a DevNode. The lanes visit the same nodes in the same order, two to a trip: hits, frames and counters are unchanged.
template <bool STATS, bool GB = false, class STK> DEV void trav_step_inner_fast(Trav &T, const DevBvh &bvh, STK &stk, float min_dst, LaneStats<STATS> &st) {
    typedef float f3v __attribute__((ext_vector_type(3)));
    const float4 *p = reinterpret_cast<const float4 *>(bvh.nodes + T.cur);
    const float4 r0 = p[0], r1 = p[1], r2 = p[2];
    const f3v r3 = *reinterpret_cast<const f3v *>(p + 3); // left right sel
    const NodeRec n = node_rec(r0, r1, r2, r3);
    trav_inner_apply<STATS, GB, true>(T, stk, n, min_dst, st);
    if (bvh.compact == nullptr) // wave-uniform
        return;
    const bool went_left = T.cur == n.left; // else n.right or T_POP
    const uint32_t sel = __float_as_uint(r3.z) >> (went_left ? 0u : RT_SEL_RIGHT_SHIFT);
    const bool second = ((T.cur & RT_LEAF_FLAG) == 0u) & ((sel & RT_SEL_VALID) != 0u); // (T_POP has the leaf bit)
    if (__ballot(second) == 0ull)
        return;
    if (second) {
        V3 bmin = went_left ? n.lmin : n.rmn, bmax = went_left ? n.lmax : n.rmx;
        // the parent's other ten planes die here, before the compact record arrives (the scheduler would hoist its loads above the selects)
        asm volatile("" : "+v"(bmin.x), "+v"(bmin.y), "+v"(bmin.z), "+v"(bmax.x), "+v"(bmax.y), "+v"(bmax.z)::"memory");
        const float4 *c = reinterpret_cast<const float4 *>(bvh.compact + T.cur);
        const float4 c0 = c[0], c1 = c[1];
        st.second();
        trav_inner_apply<STATS, GB, true>(T, stk, node_rec_compact(c0, c1, bmin, bmax, sel), min_dst, st);
    }
}
// one unwind step for every lane in T_POP, as straight-line wave code (lanes in other states pass through unchanged)
template <bool GB = false, class STK> DEV void trav_pop_once(Trav &T, STK &stk) {
    const bool pop = T.cur == T_POP;
    const bool go = pop & (T.sp != 0);
    const int nsp = T.sp - 1;
    const bool refill = go & (nsp > 0);
    uint32_t n_ref;
    float n_d, n_loc = 0.0f;
    stk.pop_masked(nsp - 1, refill, n_ref, n_d, n_loc);
    const float t_near = T.t_loc;
    // reference: !has || t_near > d_far against the NEAR subtree's local best (bvh.h:221); GB: against the global best
    const bool visit = !(t_near <= T.top_d);
    T.cur = pop ? (go ? (visit ? T.top_ref : T_POP) : T_DONE) : T.cur;
    if constexpr (!GB)
        T.t_loc = go ? fminf(T.top_loc, t_near) : t_near;
    T.sp = go ? nsp : T.sp;
    T.top_ref = refill ? n_ref : T.top_ref;
    T.top_d = refill ? n_d : T.top_d;
    if constexpr (!GB)
        T.top_loc = refill ? n_loc : T.top_loc;
}
template <bool GB = false, class STK> DEV void trav_pop_wave(Trav &T, STK &stk) {
    while (__ballot(T.cur == T_POP) != 0ull)
        trav_pop_once<GB>(T, stk);
}
// ---------------------------------------------------------------------------------------------- cooperative triangle batch
// The triangles several lanes of a wave wait on, tested by ALL 64 lanes: the waiting lanes' (ray, triangle) pairs are laid out densely over
// the wave (prefix sum of the per-lane counts n <= N_ENT), each lane fetches "its" ray from the owning lane with cross-lane reads and runs
// one triangle test; a lane's result is the minimum of a 64-bit key (t bits, record) over its pairs, reduced with LDS atomics: smallest t
// and, on equal t, the lowest record — for records in leaf order exactly the leaf loop's strict-less replacement order (bvh.h:200-204,132).
// The callers supply what differs between the trees:
//   entry(t)      : 8-bit code of the lane's t-th pending triangle, called for t = 0 .. N_ENT - 1 in this order (it may keep state)
//   addr(base, e) : index into `recs` of the triangle with code e of a lane whose `base` is given; also the low word of the key
//   PAYLOAD       : what the leading pair publishes next to the key: float2 {b, c}, or float4 {b, c, TriRec::index, -}
// and read their own result back with coop_result.
template <class PAYLOAD> struct CoopLds { // one wave's window
    uint16_t *owner;           // [64 * N_ENT + N_ENT]: + overshoot of the unpredicated owner stores
    unsigned long long *min;   // [64]
    PAYLOAD *pay;              // [64]
};
template <class PAYLOAD> DEV PAYLOAD coop_payload(V3 xs, uint32_t index) {
    if constexpr (sizeof(PAYLOAD) == sizeof(float2))
        return make_float2(xs.x, xs.y);
    else
        return make_float4(xs.x, xs.y, __uint_as_float(index), 0.0f);
}
template <int N_ENT, bool STATS, class PAYLOAD, class REC, class ENTRY, class ADDR>
DEV void coop_tri_batch(bool waiting, uint32_t n, uint32_t base, V3 ro, V3 rd, const REC *recs, const CoopLds<PAYLOAD> &lds, ENTRY entry, ADDR addr, LaneStats<STATS> &st) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t total;
    const uint32_t off = wave_prefix_sum4(n, total);
    // Owner table: position off + t belongs to (lane, entry(t)) for t < n. Every waiting lane writes ALL N_ENT
    // entries, highest t first, without a per-entry predicate: an entry with t >= n lands on position off' + t' of a
    // later lane (off' > off, hence t' < t), whose own store of that position is issued LATER (a wave's LDS
    // instructions execute in order) and wins; within one instruction the waiting lanes' positions are distinct
    // (their offsets increase strictly). Positions >= total are never read; the table has room for the overshoot.
    if (waiting) {
        uint16_t ent[N_ENT];
#pragma unroll
        for (int t = 0; t < N_ENT; ++t)
            ent[t] = (uint16_t)(lane | (entry(t) << 8));
#pragma unroll
        for (int t = N_ENT - 1; t >= 0; --t) {
            lds.owner[off + t] = ent[t];
            asm volatile("" ::: "memory"); // keep the stores in this order (compiler and machine scheduler)
        }
        lds.min[lane] = ~0ull;
    }
    __threadfence_block();
    for (uint32_t q0 = 0; q0 < total; q0 += 64u) { // wave-uniform trip count
        const uint32_t q = q0 + lane;
        const bool valid = q < total;
        const uint32_t ow = valid ? (uint32_t)lds.owner[q] : 0u;
        const int src = (int)(ow & 63u);
        const uint32_t kk = addr((uint32_t)__shfl((int)base, src), ow >> 8);
        const V3 o = mk(__shfl(ro.x, src), __shfl(ro.y, src), __shfl(ro.z, src));
        const V3 d = mk(__shfl(rd.x, src), __shfl(rd.y, src), __shfl(rd.z, src));
        if (valid) {
            const float4 *p = reinterpret_cast<const float4 *>(recs + kk);
            const float4 r0 = p[0], r1 = p[1], r2 = p[2];
            const TriRec tri = tri_rec(r0, r1, r2);
            st.tri();
            V3 xs;
            if (tri_hit(tri, o, d, EPS, xs)) {
                const unsigned long long key = ((unsigned long long)__float_as_uint(xs.z) << 32) | (unsigned long long)kk;
                atomicMin(&lds.min[src], key);
                __threadfence_block();
                if (lds.min[src] == key) // this pair leads its lane's pairs so far: publish its payload
                    lds.pay[src] = coop_payload<PAYLOAD>(xs, tri.index);
            }
        }
    }
    __threadfence_block();
}
// a waiting lane's result of the batch: false = none of its triangles was hit
template <class PAYLOAD> DEV bool coop_result(const CoopLds<PAYLOAD> &lds, float &t, uint32_t &rec, PAYLOAD &pay) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long key = lds.min[lane];
    if (key == ~0ull)
        return false;
    t = __uint_as_float((uint32_t)(key >> 32));
    rec = (uint32_t)key;
    pay = lds.pay[lane];
    return true;
}

// ---------------------------------------------------------------------------------------------- light pdf
// bvh_mix_dist::pdf (raytracer.h:363-375) = BVH::foreach_intersection (bvh.h:237-260) over the light BVH summing
// triangle_dist::pdf_at (raytracer.h:255-261) in DFS order (node objects, left subtree, right subtree).
// Where the light BVH is read from: its device arrays, or the copy wf_shade stages in LDS when the tree is small
// (DevBvh::lds_inner). The records are the same 16-byte pieces either way.
struct LightTabs {
    const float4 *nodes, *tris, *aux; // DevNode = 4, DevTri = 3, DevLightAux = 1 pieces per record
};
DEV LightTabs light_tabs_global(const DevScene &S) {
    return LightTabs{reinterpret_cast<const float4 *>(S.lights.nodes), reinterpret_cast<const float4 *>(S.lights.tris), reinterpret_cast<const float4 *>(S.light_aux)};
}
template <bool STATS, class STK> DEV float lights_pdf(const DevScene &S, const LightTabs &LT, V3 x, V3 d, STK &stk, LaneStats<STATS> &st) {
    const DevBvh &bvh = S.lights;
    st.lq();
    float res = 0;
    if (bvh.root != RT_NONE && bvh.n_tris != 0) {
        uint32_t cur = bvh.root;
        int sp = 0;
        const bool fast = ray_fast_ok(bvh, x, d); // same exact-quotient shortcut as the closest-hit traversal
        const V3 r = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        while (cur != T_DONE) {
            const bool leaf = (cur & RT_LEAF_FLAG) != 0;
            const float4 *p = leaf ? LT.tris + 3u * (cur & RT_LEAF_BEGIN_MASK) : LT.nodes + 4u * cur;
            const float4 r0 = p[0], r1 = p[1], r2 = p[2];
            if (!leaf) {
                const NodeRec n = node_rec(r0, r1, r2, p[3]);
                st.lnode();
                st.lbox(2);
                const TwoBox bx = two_box(n, x, d, r, fast, EPS); // no order, no cull: every hit child is visited (bvh.h:237-260)
                if (bx.hl & bx.hr) {
                    stk.push_ref(sp++, n.right);
                    cur = n.left;
                } else if (bx.hl) {
                    cur = n.left;
                } else if (bx.hr) {
                    cur = n.right;
                } else {
                    cur = T_POP;
                }
            } else {
                const uint32_t k = cur & RT_LEAF_BEGIN_MASK;
                const TriRec tri = tri_rec(r0, r1, r2);
                const uint32_t flags = tri.flags;
                if (flags & 2u)
                    st.lnode();
                st.ltri();
                V3 xs;
                if (tri_hit(tri, x, d, EPS, xs)) {
                    st.lhit();
                    const float4 aux = LT.aux[k];
                    V3 y = x + d * xs.z;  // ray.at(t)
                    V3 dir = norm(y - x); // raytracer.h:259
                    float mult = len2(x - y) / __builtin_fabsf(dot(dir, mk(aux.x, aux.y, aux.z))); // :79-84
                    res += mult / aux.w;
                }
                cur = (flags & 1u) ? T_POP : cur + 1;
            }
            if (cur == T_POP)
                cur = sp ? stk.pop_ref(--sp) : T_DONE;
        }
    }
    return res / (float)bvh.n_tris; // res / bvh->objects.size()
}

} // namespace
