// rt_update_dev.hip — rt_update_geometry_device's look at arrays that are in HBM already: what rt_update_geometry finds out with two host loops
// over the arrays (check_update's refusals, rt_update.cpp; prepare_geometry's pick of the emissive triangles, rt_scene.cpp), by one streaming
// pass and a stable compaction on the device. 40 bytes per triangle are read once (positions 36, material id 4), the ids a second time.
//
//   scan      a block takes chunks of 256 triangles, grid-stride. The 2304 position floats of a chunk are read as a flat run (lane t reads
//             floats t, t + 256, ...: whole cache lines per wave whatever the arrays' alignment beyond 4 bytes); float j of a chunk is
//             component (j mod 3) of triangle j / 9, so a lane folds it into one of three running minima / maxima. Thread t also judges
//             material id t of the chunk: in range, and emissive by the per-material byte table. Per chunk the block stores its count of
//             emissive triangles; per wave, at the end, the bounds go to k_bounds' words (ordered-integer atomicMin / atomicMax), the lowest
//             triangle with a non-finite float to an atomicMin, "an id was out of range" to an atomicOr.
//   offsets   rocPRIM's exclusive scan of the per-chunk counts.
//   compact   the same chunks again: an emissive triangle's rank within its chunk (ballot + popcount, wave bases through LDS) added to the
//             chunk's offset is its place in the output, where its index and its nine position floats go.
// Integer min / max / or commute and min / max of floats are exact, so every word is the same whichever block runs first; the compaction
// writes each light to a place that follows from the arrays alone. No float atomics, no order-dependent output.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_build_dev.h"
#include "rt_build_scan.h"
#include "rt_kernels.h"
#include "rt_update_dev.h"

namespace {

constexpr uint32_t CHUNK = 256; // triangles per chunk = threads per block

struct ScanArgs {
    const float *pos;
    const uint32_t *mat;
    const uint8_t *emissive; // [n_mats]
    uint32_t n, n_mats, n_chunks;
    uint32_t *words;         // [0..5] k_bounds' words, [6] lowest triangle with a non-finite float (RT_NONE: none), [7] != 0: an id >= n_mats
    uint32_t *chunk_lights;  // [n_chunks] emissive triangles of the chunk
    // compaction
    const uint32_t *chunk_first; // [n_chunks] exclusive scan of chunk_lights
    uint32_t n_lights;
    uint32_t *out_prim; // [n_lights]
    float *out_pos;     // [n_lights][9]
};

// thread t's triangle of the chunk: is it emissive? (`bad` is set for an id outside the table, which is then not read)
__device__ __forceinline__ bool chunk_emissive(const ScanArgs &A, uint32_t chunk, uint32_t &tri, bool &bad) {
    const uint64_t i = (uint64_t)CHUNK * chunk + threadIdx.x;
    tri = (uint32_t)i;
    if (i >= A.n || !A.mat) // no ids (a scan of positions alone): nothing is emissive
        return false;
    const uint32_t id = A.mat[i];
    if (id >= A.n_mats) {
        bad = true;
        return false;
    }
    return A.emissive[id] != 0;
}

__global__ __launch_bounds__(256) void k_update_scan(const ScanArgs A) {
    __shared__ uint32_t s_cnt[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t total = 9ull * A.n;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    uint32_t bad_tri = RT_NONE;
    bool bad_mat = false;
    const uint32_t c0 = t % 3u;
    for (uint32_t chunk = blockIdx.x; chunk < A.n_chunks; chunk += gridDim.x) {
        const uint64_t base = 9ull * CHUNK * chunk;
#pragma unroll
        for (uint32_t k = 0; k < 9u; ++k) {
            const uint32_t j = t + CHUNK * k; // float j of the chunk: CHUNK mod 3 == 1, so its component is (t + k) mod 3
            if (base + j < total) {
                const float f = A.pos[base + j];
                const uint32_t c = (c0 + k) % 3u;
#pragma unroll
                for (uint32_t q = 0; q < 3u; ++q) {
                    lo[q] = c == q ? fminf(lo[q], f) : lo[q];
                    hi[q] = c == q ? fmaxf(hi[q], f) : hi[q];
                }
                if ((__float_as_uint(f) & 0x7F800000u) == 0x7F800000u) // NaN or infinity
                    bad_tri = min(bad_tri, CHUNK * chunk + j / 9u);
            }
        }
        uint32_t tri;
        const bool em = chunk_emissive(A, chunk, tri, bad_mat);
        const uint32_t cnt = (uint32_t)__popcll(__ballot(em));
        if (lane == 0u)
            s_cnt[wave] = cnt;
        __syncthreads();
        if (t == 0u)
            A.chunk_lights[chunk] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        for (int off = 32; off > 0; off >>= 1) {
            lo[c] = fminf(lo[c], __shfl_down(lo[c], off));
            hi[c] = fmaxf(hi[c], __shfl_down(hi[c], off));
        }
    for (int off = 32; off > 0; off >>= 1)
        bad_tri = min(bad_tri, (uint32_t)__shfl_down((int)bad_tri, off));
    const bool any_bad_mat = __any(bad_mat) != 0;
    if (lane == 0u) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            atomicMin(A.words + c, enc_f(lo[c]));
            atomicMax(A.words + 3 + c, enc_f(hi[c]));
        }
        if (bad_tri != RT_NONE)
            atomicMin(A.words + 6, bad_tri);
        if (any_bad_mat)
            atomicOr(A.words + 7, 1u);
    }
}

__global__ __launch_bounds__(256) void k_update_compact(const ScanArgs A) {
    __shared__ uint32_t s_cnt[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (uint32_t chunk = blockIdx.x; chunk < A.n_chunks; chunk += gridDim.x) {
        uint32_t tri;
        bool bad = false;
        const bool em = chunk_emissive(A, chunk, tri, bad);
        const unsigned long long m = __ballot(em);
        if (lane == 0u)
            s_cnt[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t dst = A.chunk_first[chunk] + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        for (uint32_t w = 0; w < wave; ++w)
            dst += s_cnt[w];
        // (dst < n_lights always, unless the caller changed the ids between the two kernels: then nothing is written out of bounds)
        if (em && dst < A.n_lights) {
            A.out_prim[dst] = tri;
#pragma unroll
            for (int j = 0; j < 9; ++j)
                A.out_pos[9ull * dst + j] = A.pos[9ull * tri + j];
        }
        __syncthreads();
    }
}

} // namespace

namespace rt {

hipError_t scan_update_device(const DeviceArrays &in, const std::vector<uint8_t> &emissive, bool want_lights, hipStream_t stream, UpdateScan *out, const char **err) {
    *out = UpdateScan{};
    const uint32_t n = in.n;
    if (n == 0)
        return hipSuccess;
    ScratchArena tmp{stream}; // scratch of the scan: every return path leaves no kernel running on it or on the caller's arrays
    ScanArgs A{};
    A.pos = in.pos, A.mat = in.mat, A.n = n;
    A.n_mats = (uint32_t)emissive.size();
    A.n_chunks = (uint32_t)(((uint64_t)n + CHUNK - 1) / CHUNK);
    uint8_t *d_em;
    uint32_t *chunk_first;
    ExclusiveScan scan;
    HIP_TRY_ERR(tmp.alloc(&d_em, emissive.size()));
    HIP_TRY_ERR(tmp.alloc(&A.words, (size_t)8));
    HIP_TRY_ERR(tmp.alloc(&A.chunk_lights, (size_t)A.n_chunks));
    HIP_TRY_ERR(tmp.alloc(&chunk_first, (size_t)A.n_chunks));
    HIP_TRY_ERR(scan.prepare(tmp, A.chunk_lights, chunk_first, (size_t)A.n_chunks, stream));
    A.emissive = d_em;
    static const uint32_t init_words[8] = {RT_BOUNDS_WORDS_INIT, RT_NONE, 0u};
    HIP_TRY_ERR(hipMemcpyAsync(A.words, init_words, sizeof(init_words), hipMemcpyHostToDevice, stream));
    if (!emissive.empty())
        HIP_TRY_ERR(hipMemcpyAsync(d_em, emissive.data(), emissive.size(), hipMemcpyHostToDevice, stream)); // (the caller's vector outlives the call)
    const dim3 grid(std::min<uint32_t>(A.n_chunks, 256u * 16u));
    HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_update_scan, grid, dim3(CHUNK), 0, stream, A));
    HIP_TRY_ERR(scan.run(A.chunk_lights, chunk_first, (size_t)A.n_chunks, stream));
    uint32_t h_words[8];
    uint64_t n_lights;
    HIP_TRY_ERR(hipMemcpyAsync(h_words, A.words, sizeof(h_words), hipMemcpyDeviceToHost, stream));
    HIP_TRY_ERR(scan_total(A.chunk_lights, chunk_first, (size_t)A.n_chunks, stream, &n_lights)); // synchronises: h_words is here too
    out->bad_material = h_words[7] != 0u;
    out->first_non_finite = h_words[6];
    bounds_decode(h_words, out->lo, out->hi);
    if (out->bad_material || out->first_non_finite != RT_NONE || !want_lights || n_lights == 0)
        return hipSuccess;
    if (n_lights > n) {
        if (err)
            *err = "update scan: more lights than triangles";
        return hipErrorUnknown;
    }
    A.chunk_first = chunk_first;
    A.n_lights = (uint32_t)n_lights;
    HIP_TRY_ERR(tmp.alloc(&A.out_prim, (size_t)n_lights));
    HIP_TRY_ERR(tmp.alloc(&A.out_pos, 9ull * n_lights));
    out->light_prims.resize(n_lights);
    out->light_pos.resize(9ull * n_lights);
    HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_update_compact, grid, dim3(CHUNK), 0, stream, A));
    HIP_TRY_ERR(hipMemcpyAsync(out->light_prims.data(), A.out_prim, 4ull * n_lights, hipMemcpyDeviceToHost, stream));
    HIP_TRY_ERR(hipMemcpyAsync(out->light_pos.data(), A.out_pos, 36ull * n_lights, hipMemcpyDeviceToHost, stream));
    HIP_TRY_ERR(hipStreamSynchronize(stream));
    return hipSuccess;
}

} // namespace rt
