// rt_wide_refit.hip — the packed 8-wide tree refitted to new triangle arrays (rt_update_geometry, RT_UPDATE_REFIT): same topology, new boxes.
//
// The packed tree (rt_device_types.h, "what the wide kernels READ") has a fixed topology: group bases, slot states and the order of the
// triangle records say who is below whom. Everything else in it — node origins, cell exponents, the 48 plane bytes, the triangle records — is
// a pure function of that topology and of the positions. This file recomputes that function:
//   records    one lane per triangle record k: DevTri[k] / DevAttr[k] again from the raw arrays at prim = DevTri[k].prim (tri_records, the
//              arithmetic of k_leaves), and the triangle's exact vertex box
//   levels     top down from the root, one launch per level: every node gets a dense id, its unit index and the id of its first inner child
//              (the host reads one counter per level, as the device collapse does)
//   nodes      bottom up, one launch per level: a lane gathers the exact boxes of its node's slots (leaf slots from the triangle boxes, inner
//              slots from the boxes its children wrote one launch earlier), forms the node box with min / max, then origin, exponents and
//              planes by the builders' rule (wide_grid.h: wide_node_frame, wide_quantise_axis — the code k_wide_emit runs), writes header and
//              planes, copies the refreshed triangle records of its leaf slots behind its children, and leaves its own box for its parent.
// A child's box reaches its parent across a kernel boundary, so no fence, flag or atomic orders anything here (the only atomic hands out
// ids in the top-down pass, and the ids cancel out of every result). Which lane computes a node, and when, changes nothing.
// The refit is a model-checked copy of rt::refit_wide (wide_build.cpp): tests compare the two byte for byte.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "rt_build_dev.h"
#include "rt_build_host.h"
#include "rt_kernels.h"
#include "rt_wide_refit.h"
#include "wide_grid.h"

namespace {

struct RefitArgs {
    const float *pos, *nrm, *tan, *uv;
    const uint32_t *mat;
    DevTri *tris;
    DevAttr *attrs;
    uint32_t n_tris;
    uint4 *blob;
    uint32_t n_units, n_wide;
    float *tri_box;        // [n_tris][6]
    float *node_box;       // [n_wide][6], by dense id
    uint32_t *node_unit;   // [n_wide]: unit index of the node's record
    uint32_t *child_first; // [n_wide]: dense id of its first inner child
    uint32_t *counters;    // [0] ids handed out, [1] set when the blob contradicts n_wide / n_units / n_tris (nothing is written out of bounds)
    uint32_t first, count; // this launch's level: ids [first, first + count)
    WideGrid grid;
};

__global__ __launch_bounds__(256) void k_refit_records(const RefitArgs A) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= A.n_tris)
        return;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    bool ok = true;
    DevTri t;
    DevAttr at;
    tri_records(A.pos, A.nrm, A.tan, A.uv, A.mat, A.tris[k].prim, t, at, lo, hi, ok);
    A.tris[k] = t;
    A.attrs[k] = at;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        A.tri_box[6ull * k + c] = lo[c];
        A.tri_box[6ull * k + 3 + c] = hi[c];
    }
}

__device__ __forceinline__ uint32_t inner_slots(uint32_t state) { // slots in state 100
    uint32_t n = 0;
#pragma unroll
    for (uint32_t s = 0; s < 8u; ++s)
        n += ((state >> (3u * s)) & 7u) == 4u ? 1u : 0u;
    return n;
}

__global__ __launch_bounds__(256) void k_refit_level(const RefitArgs A) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= A.count)
        return;
    const uint32_t id = A.first + q, u = A.node_unit[id];
    const uint4 h = A.blob[u];
    const uint32_t n_inner = inner_slots(h.y & 0xFFFFFFu);
    uint32_t first = 0u;
    if (n_inner) {
        first = atomicAdd(A.counters + 0, n_inner);
        if ((uint64_t)first + n_inner > A.n_wide || (uint64_t)h.x + RT_WIDE_NODE_UNITS * n_inner > A.n_units) {
            A.counters[1] = 1u;
            A.child_first[id] = RT_NONE;
            return;
        }
        for (uint32_t r = 0; r < n_inner; ++r)
            A.node_unit[first + r] = h.x + RT_WIDE_NODE_UNITS * r;
    }
    A.child_first[id] = first;
}

__global__ __launch_bounds__(64) void k_refit_nodes(const RefitArgs A) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= A.count)
        return;
    const uint32_t id = A.first + q, u = A.node_unit[id];
    const uint4 h = A.blob[u];
    const uint32_t state = h.y & 0xFFFFFFu, n_inner = inner_slots(state), cfirst = A.child_first[id];
    const uint32_t tu = h.x + RT_WIDE_NODE_UNITS * n_inner; // the node's triangle records
    if (cfirst == RT_NONE)
        return; // flagged by k_refit_level
    // ---- the exact boxes of the slots, and the refreshed triangle records of the leaf slots
    float sbox[8][6];
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    uint32_t r_inner = 0, r_tri = 0;
#pragma unroll
    for (uint32_t s = 0; s < 8u; ++s) {
        const uint32_t code = (state >> (3u * s)) & 7u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sbox[s][c] = __builtin_inff();
            sbox[s][3 + c] = -__builtin_inff();
        }
        if (code == 4u) {
            const float *b = A.node_box + 6ull * (cfirst + r_inner);
            ++r_inner;
#pragma unroll
            for (int c = 0; c < 6; ++c)
                sbox[s][c] = b[c];
        } else if (code != 0u) {
            const uint32_t cnt = (uint32_t)__popc(code);
            for (uint32_t j = 0; j < cnt; ++j, ++r_tri) {
                const uint64_t at = (uint64_t)tu + RT_WIDE_TRI_UNITS * r_tri;
                if (at + RT_WIDE_TRI_UNITS > A.n_units) {
                    A.counters[1] = 1u;
                    return;
                }
                const uint32_t k = A.blob[at + 2].w; // DevTri::pad of a record in the blob: its index into DevTri[] / DevAttr[]
                if (k >= A.n_tris) {
                    A.counters[1] = 1u;
                    return;
                }
                const uint4 *t = reinterpret_cast<const uint4 *>(A.tris + k);
                uint4 r2 = t[2];
                r2.w = k;
                A.blob[at] = t[0];
                A.blob[at + 1] = t[1];
                A.blob[at + 2] = r2;
                const float *b = A.tri_box + 6ull * k;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    sbox[s][c] = fminf(sbox[s][c], b[c]);
                    sbox[s][3 + c] = fmaxf(sbox[s][3 + c], b[3 + c]);
                }
            }
        } else
            continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = fminf(lo[c], sbox[s][c]);
            hi[c] = fmaxf(hi[c], sbox[s][3 + c]);
        }
    }
    // ---- the node's own grid, then every occupied slot's planes on it; empty slots keep the inverted box (255, 0)
    float org[3];
    int ecell[3];
    wide_node_frame(A.grid, lo, hi, org, ecell);
    uint32_t pl[12]; // the 48 plane bytes as WideNode::qlo[3][8], qhi[3][8]: qlo[c][s] is byte s & 3 of word 2 c + (s >> 2), qhi six words on
#pragma unroll
    for (int w = 0; w < 6; ++w) {
        pl[w] = 0xFFFFFFFFu;
        pl[6 + w] = 0u;
    }
#pragma unroll
    for (uint32_t s = 0; s < 8u; ++s) {
        if (((state >> (3u * s)) & 7u) == 0u)
            continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint8_t ql, qh;
            wide_quantise_axis(org[c], ecell[c], sbox[s][c], sbox[s][3 + c], &ql, &qh);
            const uint32_t w = 2u * (uint32_t)c + (s >> 2), sh = 8u * (s & 3u);
            pl[w] = (pl[w] & ~(0xFFu << sh)) | ((uint32_t)ql << sh);
            pl[6 + w] |= (uint32_t)qh << sh;
        }
    }
    uint32_t m[3], e4[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        (void)wide_snap_origin(A.grid, c, org[c], &m[c]); // org is on the grid: this recovers its index, as the pack pass does
        const int e = ecell[c] - A.grid.e_base;
        e4[c] = (uint32_t)(e < 0 ? 0 : (e > 15 ? 15 : e));
    }
    uint4 hdr;
    hdr.x = h.x;
    hdr.y = state | (e4[0] << 24) | (e4[1] << 28);
    hdr.z = m[0] | (m[1] << 20);
    hdr.w = (m[1] >> 12) | (m[2] << 8) | (e4[2] << 28);
    A.blob[u] = hdr;
    A.blob[u + 1] = make_uint4(pl[0], pl[1], pl[2], pl[3]);
    A.blob[u + 2] = make_uint4(pl[4], pl[5], pl[6], pl[7]);
    A.blob[u + 3] = make_uint4(pl[8], pl[9], pl[10], pl[11]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        A.node_box[6ull * id + c] = lo[c];
        A.node_box[6ull * id + 3 + c] = hi[c];
    }
}

} // namespace

namespace rt {

hipError_t refit_upload(const rt_geometry_update *upd, hipStream_t stream, RefitInput *in, const char **err) {
    const uint32_t n = upd->n_triangles;
    *in = RefitInput{};
    in->n = n;
    if (n == 0)
        return hipSuccess;
    HIP_TRY_ERR(in->owned.alloc_bytes(&in->pos, 36ull * n));
    HIP_TRY_ERR(in->owned.alloc_bytes(&in->nrm, 36ull * n));
    HIP_TRY_ERR(in->owned.alloc_bytes(&in->tan, 36ull * n));
    HIP_TRY_ERR(in->owned.alloc_bytes(&in->uv, 24ull * n));
    HIP_TRY_ERR(in->owned.alloc_bytes(&in->mat, 4ull * n));
    HIP_TRY_ERR(in->owned.alloc_bytes(&in->bounds, 8 * sizeof(uint32_t)));
    const uint32_t init_bounds[8] = {RT_BOUNDS_WORDS_INIT, 0u, 0u};
    HIP_TRY_ERR(hipMemcpyAsync(in->pos, upd->positions, 36ull * n, hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipMemcpyAsync(in->nrm, upd->normals, 36ull * n, hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipMemcpyAsync(in->tan, upd->tangents, 36ull * n, hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipMemcpyAsync(in->uv, upd->texcoords, 24ull * n, hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipMemcpyAsync(in->mat, upd->material_ids, 4ull * n, hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipMemcpyAsync(in->bounds, init_bounds, sizeof(init_bounds), hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipStreamSynchronize(stream)); // `init_bounds` is a local
    const int blocks = (int)std::min<uint64_t>(((uint64_t)n + 255) / 256, 256u * 16u);
    HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_bounds, dim3(blocks), dim3(256), 0, stream, in->pos, n, in->bounds));
    uint32_t h_bounds[8];
    HIP_TRY_ERR(read_back(h_bounds, in->bounds, 8, stream));
    bounds_decode(h_bounds, in->lo, in->hi);
    return hipSuccess;
}

hipError_t refit_wide_device(const RefitInput &in, DevTri *tris, DevAttr *attrs, uint32_t n_tris, uint4_pod *blob, uint32_t n_units, uint32_t n_wide,
                             const WideGrid &grid, hipStream_t stream, const char **err, double *levels_ms) {
    if (levels_ms)
        *levels_ms = 0;
    if (n_tris == 0 || n_wide == 0)
        return hipSuccess;
    ScratchArena tmp{stream}; // scratch of the refit: drained, then freed, on every return path
    RefitArgs A{};
    A.pos = in.pos, A.nrm = in.nrm, A.tan = in.tan, A.uv = in.uv, A.mat = in.mat;
    A.tris = tris, A.attrs = attrs, A.n_tris = n_tris;
    A.blob = reinterpret_cast<uint4 *>(blob), A.n_units = n_units, A.n_wide = n_wide;
    A.grid = grid;
    // every allocation comes before the first write to anything the render kernels read
    HIP_TRY_ERR(tmp.alloc(&A.tri_box, 6ull * n_tris));
    HIP_TRY_ERR(tmp.alloc(&A.node_box, 6ull * n_wide));
    HIP_TRY_ERR(tmp.alloc(&A.node_unit, (size_t)n_wide));
    HIP_TRY_ERR(tmp.alloc(&A.child_first, (size_t)n_wide));
    HIP_TRY_ERR(tmp.alloc(&A.counters, (size_t)2));
    const uint32_t init[3] = {1u, 0u, 0u}; // id 0 = the root, at unit 0
    HIP_TRY_ERR(hipMemcpyAsync(A.counters, init, 8, hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipMemcpyAsync(A.node_unit, init + 2, 4, hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipStreamSynchronize(stream)); // `init` is a local
    // ---- levels, top down (reads the blob only)
    const auto t_levels = std::chrono::steady_clock::now();
    std::vector<uint32_t> level_first{0u}, level_count{1u};
    for (;;) {
        A.first = level_first.back(), A.count = level_count.back();
        HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_refit_level, dim3((A.count + 255u) / 256u), dim3(256), 0, stream, A));
        uint32_t h[2];
        HIP_TRY_ERR(read_back(h, A.counters, 2, stream));
        const uint32_t end = A.first + A.count;
        if (h[1] != 0u || h[0] > n_wide || h[0] < end || level_first.size() > 4096u) {
            if (err)
                *err = "wide refit: the packed tree is inconsistent";
            return hipErrorUnknown;
        }
        if (h[0] == end)
            break;
        level_first.push_back(end);
        level_count.push_back(h[0] - end);
    }
    if (level_first.back() + level_count.back() != n_wide) { // a node no parent names: still nothing has been written
        if (err)
            *err = "wide refit: the packed tree is inconsistent";
        return hipErrorUnknown;
    }
    if (levels_ms)
        *levels_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_levels).count();
    // ---- records, then nodes bottom up
    HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_refit_records, dim3((n_tris + 255u) / 256u), dim3(256), 0, stream, A));
    for (size_t l = level_first.size(); l-- > 0;) {
        A.first = level_first[l], A.count = level_count[l];
        HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_refit_nodes, dim3((A.count + 63u) / 64u), dim3(64), 0, stream, A));
    }
    uint32_t h[2];
    HIP_TRY_ERR(read_back(h, A.counters, 2, stream));
    if (h[1] != 0u) {
        if (err)
            *err = "wide refit: the packed tree is inconsistent";
        return hipErrorUnknown;
    }
    return hipSuccess;
}

} // namespace rt
