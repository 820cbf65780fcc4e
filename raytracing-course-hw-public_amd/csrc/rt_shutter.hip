// rt_shutter.hip — the device side of a shutter accumulator (rt_abi.h rt_accum_attach_shutter: the rule; rt_accum_shutter.cpp: the host side).
//
//   blend          the geometry at time t from the two keys: positions, normals and tangents, 27 floats per triangle, one launch. A stream:
//                  216 bytes read and 108 written per triangle, as 16-byte accesses (every array starts an allocation of the
//                  accumulator's arena), grid-stride over at most 2048 blocks; the floats of 9n that do not fill a float4 are the
//                  tail, one each for the first threads. Each float is its own lane's: no result depends on scheduling.
//   moving lights  does any emissive triangle have a position float whose keys differ in a bit? One word, OR-ed.
// The blend is written with __fsub_rn / __fmul_rn / __fadd_rn: three roundings whatever -ffp-contract says, as the rule states them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rt_kernels.h"
#include "rt_shutter.h"

namespace {

// x(t) of the rule for one float: b = x0 + t * (x1 - x0), then held between the keys by comparisons alone (a NaN b, from keys of opposite
// sign whose difference overflows, falls to lo; equal keys give key 0's bits, a signed zero included)
__device__ __forceinline__ float shutter_blend(float x0, float x1, float t) {
    const float b = __fadd_rn(x0, __fmul_rn(t, __fsub_rn(x1, x0)));
    const bool up = x0 <= x1;
    const float lo = up ? x0 : x1, hi = up ? x1 : x0;
    return !(b > lo) ? lo : (!(b < hi) ? hi : b);
}

struct BlendArgs {
    const float *k0[3], *k1[3];
    float *out[3];
    uint32_t n4;   // whole float4 of one array
    uint32_t tail; // floats behind them (0..3)
    float t;
};

__global__ __launch_bounds__(256) void k_shutter_blend(const BlendArgs A) {
    const uint32_t stride = gridDim.x * blockDim.x, first = blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float4 *p0 = reinterpret_cast<const float4 *>(A.k0[a]), *p1 = reinterpret_cast<const float4 *>(A.k1[a]);
        float4 *po = reinterpret_cast<float4 *>(A.out[a]);
        for (uint32_t i = first; i < A.n4; i += stride) {
            const float4 x0 = p0[i], x1 = p1[i];
            float4 r;
            r.x = shutter_blend(x0.x, x1.x, A.t);
            r.y = shutter_blend(x0.y, x1.y, A.t);
            r.z = shutter_blend(x0.z, x1.z, A.t);
            r.w = shutter_blend(x0.w, x1.w, A.t);
            po[i] = r;
        }
        if (first < A.tail) {
            const size_t j = 4ull * A.n4 + first;
            A.out[a][j] = shutter_blend(A.k0[a][j], A.k1[a][j], A.t);
        }
    }
}

__global__ __launch_bounds__(256) void k_shutter_moving_lights(const float *pos0, const float *pos1, const uint32_t *mat, const uint8_t *emissive, uint32_t n_mats,
                                                               uint32_t n, uint32_t *moving) {
    const uint32_t stride = gridDim.x * blockDim.x;
    bool moves = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t id = mat[i];
        if (id >= n_mats || emissive[id] == 0)
            continue;
#pragma unroll
        for (int j = 0; j < 9; ++j)
            moves |= __float_as_uint(pos0[9ull * i + j]) != __float_as_uint(pos1[9ull * i + j]);
    }
    if (__any(moves) && (threadIdx.x & 63u) == 0u)
        atomicOr(moving, 1u);
}

uint32_t stream_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (items + 255) / 256), 2048); }

} // namespace

namespace rt {

hipError_t launch_shutter_blend(const ShutterArrays &key0, const ShutterArrays &key1, const ShutterArrays &out, uint32_t n_triangles, float t, hipStream_t stream) {
    if (n_triangles == 0)
        return hipSuccess;
    BlendArgs A{};
    for (int a = 0; a < 3; ++a)
        A.k0[a] = key0.a[a], A.k1[a] = key1.a[a], A.out[a] = out.a[a];
    const uint64_t floats = 9ull * n_triangles; // < 2^36: n4 fits 32 bits
    A.n4 = (uint32_t)(floats / 4);
    A.tail = (uint32_t)(floats % 4);
    A.t = t;
    return RT_LAUNCH_CHECKED(k_shutter_blend, dim3(stream_grid(A.n4)), dim3(256), 0, stream, A);
}

hipError_t launch_shutter_moving_lights(const float *pos0, const float *pos1, const uint32_t *mat, const uint8_t *d_emissive, uint32_t n_materials,
                                        uint32_t n_triangles, uint32_t *d_moving, hipStream_t stream) {
    if (n_triangles == 0)
        return hipSuccess;
    return RT_LAUNCH_CHECKED(k_shutter_moving_lights, dim3(stream_grid(n_triangles)), dim3(256), 0, stream, pos0, pos1, mat, d_emissive, n_materials, n_triangles,
                             d_moving);
}

} // namespace rt
