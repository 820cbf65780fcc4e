// rt_dev_math.h — the arithmetic every device file shares: float3 / colour algebra with the reference's operation order, wave helpers, the event
// counters and the RNG policies. Reference citations are next to each function.
//
// Arithmetic contract: IEEE binary32, correctly rounded / and sqrt, no FMA contraction (-ffp-contract=off); FMA only
// where written explicitly (div_exact_fast). std::min/std::max operand order is reproduced by explicit selects.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_abi.h"
#include "../../include/rt_devspec.h"
#include "rt_device_types.h"

namespace {

constexpr float EPS = 1e-4;               // config.h:15
constexpr float MIN_ROUGHNESS = 0.04f;    // config.h:20
constexpr float VNDF_FACTOR = 1.0f / 3;   // config.h:26
constexpr float PI_F = 3.14159265358979323846f;
#define RT_INF __builtin_inff()
#define RT_NAN __builtin_nanf("")

#define DEV __device__ __forceinline__

struct V3 {
    float x, y, z;
};
DEV V3 mk(float x, float y, float z) { return V3{x, y, z}; }
DEV V3 ld3(const float *p) { return V3{p[0], p[1], p[2]}; }
DEV V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
DEV V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
DEV V3 operator*(V3 a, V3 b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
DEV V3 operator/(V3 a, V3 b) { return {a.x / b.x, a.y / b.y, a.z / b.z}; }
DEV V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
DEV V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
DEV V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
DEV V3 operator/(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
DEV V3 operator-(float s, V3 a) { return {s - a.x, s - a.y, s - a.z}; }
DEV V3 operator-(V3 a, float s) { return {a.x - s, a.y - s, a.z - s}; }
DEV float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
DEV float len2(V3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
DEV float len(V3 a) { return __builtin_sqrtf(len2(a)); }
DEV V3 crs(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; } // geometry.h:18-24
DEV V3 norm(V3 v) { return v / len(v); }                                                                   // geometry.h:31-34
DEV float rmin(float a, float b) { return (b < a) ? b : a; } // std::min(a,b)
DEV float rmax(float a, float b) { return (a < b) ? b : a; } // std::max(a,b)
DEV V3 transform3(V3 l, V3 x, V3 y, V3 z) { return l.x * x + l.y * y + l.z * z; } // geometry.h:355-359
DEV float pow2(float x) { return x * x; }
DEV float pow5(float x) { // raytracer.h:28-38, p = 5
    float x2 = x * x;
    return x * ((x2 * x2) * 1.0f);
}
DEV bool isnan_f(float x) { return x != x; }
// number of set bits of a ballot below this lane: the lane's rank among the ballot's lanes
DEV uint32_t lane_rank(unsigned long long mask) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u)); }
// exclusive prefix sum over the wave of a per-lane count n < 16, one ballot per bit plane; `total`: the wave's sum
DEV uint32_t wave_prefix_sum4(uint32_t n, uint32_t &total) {
    uint32_t off = 0;
    total = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const unsigned long long m = __ballot((n >> b) & 1u);
        off += lane_rank(m) << b;
        total += (uint32_t)__popcll(m) << b;
    }
    return off;
}

struct C4 {
    float r, g, b, a;
};
DEV C4 operator*(float s, C4 c) { return {s * c.r, s * c.g, s * c.b, s * c.a}; }
DEV C4 operator+(C4 a, C4 b) { return {a.r + b.r, a.g + b.g, a.b + b.b, a.a + b.a}; }
DEV C4 operator*(C4 a, C4 b) { return {a.r * b.r, a.g * b.g, a.b * b.b, a.a * b.a}; }

// ---------------------------------------------------------------------------------------------- wave helpers
// Scalar (s_load) reads of scene constants at a wave-uniform address: the constant address space tells the compiler that
// nothing in the kernel writes them.
typedef float F4v __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) F4v *ConstF4;
DEV ConstF4 as_const_f4(const void *p) { return (ConstF4)(unsigned long long)p; }
// minimum of a value over the 64 lanes of a fully active wave (row shifts, then the two row broadcasts of gfx9 DPP)
DEV uint32_t wave_min_u32(uint32_t v) {
    const int id = -1; // 0xFFFFFFFF: what a lane without a source reads
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x111, 0xF, 0xF, false)); // row_shr:1
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x112, 0xF, 0xF, false)); // row_shr:2
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x114, 0xF, 0xF, false)); // row_shr:4
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x118, 0xF, 0xF, false)); // row_shr:8 -> lane 15 of a row = row minimum
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x142, 0xA, 0xF, false)); // row_bcast:15 into rows 1 and 3
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x143, 0xC, 0xF, false)); // row_bcast:31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// ---------------------------------------------------------------------------------------------- counters
template <bool ON> struct LaneStats;
template <> struct LaneStats<false> {
    DEV void cast() {}
    DEV void node() {}
    DEV void box(uint32_t) {}
    DEV void tri() {}
    DEV void shaded() {}
    DEV void lq() {}
    DEV void lnode() {}
    DEV void lbox(uint32_t) {}
    DEV void ltri() {}
    DEV void lhit() {}
    DEV void texels(uint32_t) {}
    DEV void sample() {}
    DEV void second() {}
    DEV void flush(DevStats *) {}
};
template <> struct LaneStats<true> {
    unsigned long long c_cast = 0, c_node = 0, c_box = 0, c_tri = 0, c_shaded = 0, c_lq = 0, c_lnode = 0, c_lbox = 0, c_ltri = 0, c_lhit = 0,
                       c_tex = 0, c_sample = 0, c_second = 0;
    DEV void cast() { ++c_cast; }
    DEV void node() { ++c_node; }
    DEV void box(uint32_t n) { c_box += n; }
    DEV void tri() { ++c_tri; }
    DEV void shaded() { ++c_shaded; }
    DEV void lq() { ++c_lq; }
    DEV void lnode() { ++c_lnode; }
    DEV void lbox(uint32_t n) { c_lbox += n; }
    DEV void ltri() { ++c_ltri; }
    DEV void lhit() { ++c_lhit; }
    DEV void texels(uint32_t n) { c_tex += n; }
    DEV void sample() { ++c_sample; }
    DEV void second() { ++c_second; }
    DEV void flush(DevStats *s) {
        if (!s)
            return;
        atomicAdd(&s->casts, c_cast);
        atomicAdd(&s->nodes, c_node);
        atomicAdd(&s->box_tests, c_box);
        atomicAdd(&s->tri_tests, c_tri);
        atomicAdd(&s->shaded, c_shaded);
        atomicAdd(&s->lq, c_lq);
        atomicAdd(&s->lnodes, c_lnode);
        atomicAdd(&s->lbox, c_lbox);
        atomicAdd(&s->ltri, c_ltri);
        atomicAdd(&s->lhits, c_lhit);
        atomicAdd(&s->texels, c_tex);
        atomicAdd(&s->samples, c_sample);
        if (c_second)
            atomicAdd(&s->second_visits, c_second);
    }
};

// ---------------------------------------------------------------------------------------------- RNG policy
template <int MODE> struct Rng;
template <> struct Rng<RT_RNG_DEVICE> {
    rt_xoshiro g;
    DEV float canonical() { return rt_xoshiro_canonical(&g); }
    DEV uint32_t below(uint32_t n) { return rt_xoshiro_below(&g, n); }
};
template <> struct Rng<RT_RNG_REFERENCE> {
    rt_minstd g;
    DEV float canonical() { return rt_minstd_canonical(&g); }
    DEV uint32_t below(uint32_t n) { return rt_minstd_below(&g, n); }
};
// std::uniform_real_distribution<float>(a, b)(rng) = canonical * (b - a) + a
template <class R> DEV float uniform_real(R &r, float a, float b) { return r.canonical() * (b - a) + a; }

} // namespace
