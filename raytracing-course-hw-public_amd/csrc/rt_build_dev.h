// rt_build_dev.h — device code the builders share: rt_bvh_device.hip builds the trees and the records, rt_wide_refit.hip recomputes them
// for new positions, rt_update_dev.hip scans them. What they must compute bit for bit alike has its one definition here, the host's reading
// of the bounds words included. Included by .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "rt_device_types.h"

namespace {

__device__ __forceinline__ uint32_t enc_f(float f) { // order-preserving float -> uint
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ float dec_f(uint32_t e) {
    const uint32_t b = (e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e;
    float f;
#if defined(__HIP_DEVICE_COMPILE__)
    f = __uint_as_float(b);
#else
    std::memcpy(&f, &b, 4);
#endif
    return f;
}

// ---- 1. bounds of all vertices: bounds[0..2] = min (encoded), bounds[3..5] = max
// What the six words hold before the first atomic (the host uploads them; a caller appends words of its own), and what they say afterwards.
#define RT_BOUNDS_WORDS_INIT 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u
inline void bounds_decode(const uint32_t *words, float lo[3], float hi[3]) {
    for (int c = 0; c < 3; ++c) {
        lo[c] = dec_f(words[c]);
        hi[c] = dec_f(words[3 + c]);
    }
}
__global__ __launch_bounds__(256) void k_bounds(const float *__restrict__ pos, uint32_t n, uint32_t *bounds) {
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float *p = pos + 9ull * i;
#pragma unroll
        for (int v = 0; v < 3; ++v)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                lo[c] = fminf(lo[c], p[3 * v + c]);
                hi[c] = fmaxf(hi[c], p[3 * v + c]);
            }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        for (int off = 32; off > 0; off >>= 1) {
            lo[c] = fminf(lo[c], __shfl_down(lo[c], off));
            hi[c] = fmaxf(hi[c], __shfl_down(hi[c], off));
        }
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            atomicMin(bounds + c, enc_f(lo[c]));
            atomicMax(bounds + 3 + c, enc_f(hi[c]));
        }
    }
}

__device__ __forceinline__ bool coord_fast_ok(float c) {
    const float m = __builtin_fabsf(c);
    return (c == 0.0f) | ((m >= 7.275957614183426e-12f) & (m <= 1099511627776.0f));
}

// The triangle record and the shading record of original triangle `prim`, from the raw arrays: the reference's operands a, b - a, c - a
// (geometry.h:473-475), its normals / tangents / uvs, base_normal() = norm(crs(v, u)) (geometry.h:477-479, 648-650) with the float operations of
// the host path (rt_scene.cpp make_attrs), its material. t.flags is the caller's (a leaf position); t.pad and at.pad are 0. The triangle's exact
// vertex box is folded into lo / hi, and `ok` is cleared when a coordinate leaves the div_exact_fast range.
__device__ __forceinline__ void tri_records(const float *__restrict__ pos, const float *__restrict__ nrm, const float *__restrict__ tan, const float *__restrict__ uv,
                                            const uint32_t *__restrict__ mat, uint32_t prim, DevTri &t, DevAttr &at, float lo[3], float hi[3], bool &ok) {
    const float *p = pos + 9ull * prim;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        t.a[c] = p[c];
        t.v[c] = p[3 + c] - p[c]; // triangle::v geometry.h:473
        t.u[c] = p[6 + c] - p[c]; // triangle::u geometry.h:475
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            lo[c] = fminf(lo[c], p[3 * v + c]);
            hi[c] = fmaxf(hi[c], p[3 * v + c]);
            ok &= coord_fast_ok(p[3 * v + c]);
        }
    }
    t.prim = prim;
    t.flags = 0;
    t.pad = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        at.n[j] = nrm[9ull * prim + j];
        at.tg[j] = tan[9ull * prim + j];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j)
        at.uv[j] = uv[6ull * prim + j];
    const float cx = t.v[1] * t.u[2] - t.v[2] * t.u[1], cy = t.v[2] * t.u[0] - t.v[0] * t.u[2], cz = t.v[0] * t.u[1] - t.v[1] * t.u[0];
    const float l = __builtin_sqrtf(cx * cx + cy * cy + cz * cz);
    at.gn[0] = cx / l;
    at.gn[1] = cy / l;
    at.gn[2] = cz / l;
    at.material = mat[prim];
    at.pad[0] = at.pad[1] = at.pad[2] = at.pad[3] = 0;
}

} // namespace
