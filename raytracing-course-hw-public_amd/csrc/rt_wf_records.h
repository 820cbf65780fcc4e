// rt_wf_records.h — the wavefront queue records as the kernels read and write them (internal, device only). rt_device_types.h describes
// WfPath, WfHit, WfFold and WfLaunch::order; this header is the ONE place that turns that description into loads, stores and bit fields.
// A record moves in 16-byte pieces (one vector-L1 access each); a reader names the pieces it needs and pays for no others.
#pragma once
#include <cstddef>

#include "rt_dev_trav.h"

static_assert(offsetof(WfPath, o) == 0 && offsetof(WfPath, dx) == 12 && offsetof(WfPath, dy) == 16 && offsetof(WfPath, path) == 24 && offsetof(WfPath, depth) == 28 &&
                  offsetof(WfPath, r) == 32 && offsetof(WfPath, fast) == 44 && offsetof(WfPath, s) == 48,
              "WfPath: piece 0 = {o, d.x}, piece 1 = {d.y, d.z, path word, depth word}, piece 2 = {1/d, fast}, piece 3 = RNG state");
static_assert(sizeof(WfHit) == 16 && offsetof(WfHit, k) == 0 && offsetof(WfHit, b) == 4 && offsetof(WfHit, c) == 8 && offsetof(WfHit, t) == 12, "WfHit: one piece {k, b, c, t}");
static_assert(sizeof(WfFold) == 16 && offsetof(WfFold, v) == 0 && offsetof(WfFold, flag) == 12, "WfFold: one piece {scale, flag} or {emission, -}");
static_assert(sizeof(rt_xoshiro) == 16 && WF_ORDER_CLASS_SHIFT == 30 && WF_ORDER_SLOT_MASK == (1u << WF_ORDER_CLASS_SHIFT) - 1u, "path / order word: slot below, class above");

// ---- WfLaunch::order entries and the path word: queue slot (or path id) in the low 30 bits, sampler class above
DEV uint32_t wf_word_slot(uint32_t w) { return w & WF_ORDER_SLOT_MASK; }
DEV uint32_t wf_word_class(uint32_t w) { return w >> WF_ORDER_CLASS_SHIFT; }
DEV uint32_t wf_word(uint32_t slot, uint32_t cls) { return slot | (cls << WF_ORDER_CLASS_SHIFT); }
DEV uint32_t wf_order_word(const WfLaunch &L, uint32_t jq) { return L.order ? L.order[jq] : jq; } // no order = identity, class 0
DEV uint32_t wf_order_slot(const WfLaunch &L, uint32_t jq) { return L.order ? wf_word_slot(L.order[jq]) : jq; }

// ---- WfPath
struct WfRay { // pieces 0..2: what a closest-hit kernel starts a traversal from
    V3 o, d, r;
    bool fast;
};
struct WfHead { // pieces 0..1: the ray without its reciprocal, and the path's bookkeeping
    V3 o, d;
    uint32_t id, cls;         // path id within the pass; sampler class of the path's next shade()
    uint32_t depth_left, nb;  // remaining trace_ray budget; pending shade() frames
};
struct WfPacked { // a whole record in registers (wf_shade computes it inside a branch and stores it behind the wave's ballot)
    float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = p0, p2 = p0;
    uint4 rng = make_uint4(0u, 0u, 0u, 0u);
};
DEV WfRay wf_load_ray(const WfPath *p) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
    const float4 p0 = q[0], p1 = q[1], p2 = q[2];
    return WfRay{mk(p0.x, p0.y, p0.z), mk(p0.w, p1.x, p1.y), mk(p2.x, p2.y, p2.z), __float_as_uint(p2.w) != 0u};
}
DEV WfHead wf_load_head(const WfPath *p) {
    const float4 *q = reinterpret_cast<const float4 *>(p);
    const float4 p0 = q[0], p1 = q[1];
    const uint32_t w = __float_as_uint(p1.z), dw = __float_as_uint(p1.w);
    return WfHead{mk(p0.x, p0.y, p0.z), mk(p0.w, p1.x, p1.y), wf_word_slot(w), wf_word_class(w), dw & 0xFFFFu, dw >> 16};
}
DEV Rng<RT_RNG_DEVICE> wf_load_rng(const WfPath *p) {
    const uint4 s = reinterpret_cast<const uint4 *>(p)[3];
    Rng<RT_RNG_DEVICE> rng;
    rng.g.s[0] = s.x, rng.g.s[1] = s.y, rng.g.s[2] = s.z, rng.g.s[3] = s.w;
    return rng;
}
// The one composition of a path record: 1 / d by IEEE division and the per-ray fast-division flag are made HERE, where the ray is made.
DEV WfPacked wf_pack(V3 o, V3 d, uint32_t id, uint32_t cls, uint32_t depth_left, uint32_t nb, const rt_xoshiro &g) {
    WfPacked k;
    k.p0 = make_float4(o.x, o.y, o.z, d.x);
    k.p1 = make_float4(d.y, d.z, __uint_as_float(wf_word(id, cls)), __uint_as_float(depth_left | (nb << 16)));
    k.p2 = make_float4(1.0f / d.x, 1.0f / d.y, 1.0f / d.z, __uint_as_float(ray_fast_ok_ray(o, d) ? 1u : 0u));
    k.rng = make_uint4(g.s[0], g.s[1], g.s[2], g.s[3]);
    return k;
}
DEV void wf_store_path(WfPath *p, const WfPacked &k) {
    float4 *q = reinterpret_cast<float4 *>(p);
    q[0] = k.p0;
    q[1] = k.p1;
    q[2] = k.p2;
    *reinterpret_cast<uint4 *>(q + 3) = k.rng;
}

// ---- WfHit. A MISS is {RT_NONE, 0, 0, 0}: t = 0, never the +inf a traversal may run with. The binary traversals (Trav) keep best.t = 0 until
// their first hit and store `best` as it is; the wide ones cull against best.t = +inf and go through wf_closed_hit first.
DEV Hit wf_miss() { return Hit{RT_NONE, 0.f, 0.f, 0.f}; }
DEV Hit wf_closed_hit(Hit h) { return Hit{h.k, h.b, h.c, h.k == RT_NONE ? 0.0f : h.t}; }
DEV void wf_store_hit(WfHit *p, const Hit &h) { *reinterpret_cast<float4 *>(p) = make_float4(__uint_as_float(h.k), h.b, h.c, h.t); }
DEV Hit wf_load_hit(const WfHit *p) {
    const float4 q = *reinterpret_cast<const float4 *>(p);
    return Hit{__float_as_uint(q.x), q.y, q.z, q.w};
}

// ---- WfFold: frame level nb of a path, `emission + inner * scale`: a scale record, and an emission record only where the emission is not
// exactly +0 (rt_device_types.h). Both arrays store their levels one after the other; the emission array follows the scale array.
DEV size_t wf_fold_index(uint32_t n_paths, uint32_t nb, uint32_t path) { return (size_t)nb * n_paths + path; }
DEV WfFold *wf_fold_scale_at(const WfLaunch &L, uint32_t nb, uint32_t path) { return L.fold + wf_fold_index(L.n_paths, nb, path); }
DEV WfFold *wf_fold_emission_at(const WfLaunch &L, uint32_t nb, uint32_t path) { return L.fold + wf_fold_index(L.n_paths, L.ray_depth + nb, path); }
DEV void wf_store_fold(const WfLaunch &L, uint32_t nb, uint32_t path, V3 emission, V3 scale) {
    const uint32_t lit = ((__float_as_uint(emission.x) | __float_as_uint(emission.y) | __float_as_uint(emission.z)) != 0u) ? 1u : 0u; // bits, not values
    *reinterpret_cast<float4 *>(wf_fold_scale_at(L, nb, path)) = make_float4(scale.x, scale.y, scale.z, __uint_as_float(lit));
    if (lit)
        *reinterpret_cast<float4 *>(wf_fold_emission_at(L, nb, path)) = make_float4(emission.x, emission.y, emission.z, 0.f);
}
DEV void wf_load_fold(const WfLaunch &L, uint32_t nb, uint32_t path, V3 &emission, V3 &scale) {
    const float4 fs = *reinterpret_cast<const float4 *>(wf_fold_scale_at(L, nb, path));
    scale = mk(fs.x, fs.y, fs.z);
    emission = mk(0.f, 0.f, 0.f); // what an unflagged frame's emission was, bit for bit
    if (__float_as_uint(fs.w) != 0u) {
        const float4 fe = *reinterpret_cast<const float4 *>(wf_fold_emission_at(L, nb, path));
        emission = mk(fe.x, fe.y, fe.z);
    }
}
