// rt_bvh_ploc.hip — the device builder's default binary tree: steps 4b / 5b of rt_bvh_device.hip, between its leaves and the collapse.
//
// PLOC (parallel locally-ordered clustering, Meister & Bittner 2018) instead of the radix tree + refit: the
// Morton-ordered leaves are clusters; every round each cluster looks RADIUS positions to either side for the neighbour whose
// union box with it has the smallest surface area, mutual nearest neighbours merge into an inner node, the survivors are
// compacted (order kept), until one cluster is left. Agglomerative with a real surface-area criterion: the tree it builds is
// close to a full SAH build where the plain LBVH only ever splits at Morton-code bits. Boxes are unions of exact boxes, so
// every stored child box is still the exact bounding box of its subtree.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rt_build_scan.h"
#include "rt_bvh_build.h"
#include "rt_kernels.h"

namespace {

struct Ploc {
    uint32_t *ref[2];   // cluster -> leaf ref / inner node index, double buffered
    float *box[2];      // [6] per cluster
    uint32_t *nn;       // nearest neighbour (cluster position)
    uint32_t *valid;    // 1 = survives this round (also holds the merged cluster), 0 = absorbed
    uint32_t *pos;      // exclusive scan of valid
    uint32_t *depth;    // per inner node: height of its subtree (leaves 0)
    uint32_t *counters; // [0] inner nodes allocated, [1] root height (written with the last merge)
    uint32_t m;         // clusters this round
    int cur;            // which buffer holds them
    int radius;
    int force;          // no mutual pair last round (cannot happen with consistent tie-breaking): pair neighbours 2k, 2k + 1
};
#define PLOC_MAX_RADIUS 32
__global__ __launch_bounds__(256) void k_ploc_nn(const Ploc P) {
    __shared__ float s_box[256 + 2 * PLOC_MAX_RADIUS][6];
    const int m = (int)P.m, R = P.radius;
    const int block0 = (int)(blockIdx.x * blockDim.x);
    const float *box = P.box[P.cur];
    for (int t = (int)threadIdx.x; t < 256 + 2 * R; t += 256) {
        const int g = block0 - R + t;
#pragma unroll
        for (int c = 0; c < 6; ++c)
            s_box[t][c] = (g >= 0 && g < m) ? box[6ull * g + c] : 0.0f;
    }
    __syncthreads();
    const int i = block0 + (int)threadIdx.x;
    if (i >= m)
        return;
    if (P.force) {
        P.nn[i] = (uint32_t)((i ^ 1) < m ? (i ^ 1) : i);
        return;
    }
    const float *bi = s_box[threadIdx.x + R];
    float best = __builtin_inff();
    int bj = i;
    for (int dj = -R; dj <= R; ++dj) {
        const int j = i + dj;
        if (dj == 0 || j < 0 || j >= m)
            continue;
        const float *bjx = s_box[threadIdx.x + R + dj];
        float u[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            u[c] = fminf(bi[c], bjx[c]);
            u[3 + c] = fmaxf(bi[3 + c], bjx[3 + c]);
        }
        const float a = box_area6(u);
        // ascending j: on equal areas the lower position wins, on both sides of a pair — except that the position's pairing partner i ^ 1 wins every
        // tie it takes part in: when ALL areas tie (clusters collapsed onto a line or a point: zero-area unions) every position would otherwise choose
        // its lowest neighbour, only positions 0 and 1 would choose each other, and a round would merge ONE pair (found by tools/soak_wide_rays.py)
        if (a < best || (a == best && j == (i ^ 1))) {
            best = a;
            bj = j;
        }
    }
    P.nn[i] = (uint32_t)bj;
}
__global__ __launch_bounds__(256) void k_ploc_merge(const Ploc P, const BuildArrays A) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.m)
        return;
    const uint32_t j = P.nn[i];
    const bool mutual = j != i && P.nn[j] == i;
    if (!mutual) {
        P.valid[i] = 1u;
        return;
    }
    if (i > j) {
        P.valid[i] = 0u; // absorbed into position j
        return;
    }
    const uint32_t lref = P.ref[P.cur][i], rref = P.ref[P.cur][j];
    float l6[6], r6[6], u[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        l6[c] = P.box[P.cur][6ull * i + c];
        r6[c] = P.box[P.cur][6ull * j + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        u[c] = fminf(l6[c], r6[c]);
        u[3 + c] = fmaxf(l6[3 + c], r6[3 + c]);
    }
    const uint32_t node = atomicAdd(P.counters + 0, 1u);
    DevNode &nd = A.nodes[node];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        nd.lmin[c] = l6[c];
        nd.lmax[c] = l6[3 + c];
        nd.rmin[c] = r6[c];
        nd.rmax[c] = r6[3 + c];
    }
    nd.left = lref;
    nd.right = rref;
    nd.sel = nd.pad = 0;
    const uint32_t dl = (lref & RT_LEAF_FLAG) ? 0u : P.depth[lref], dr = (rref & RT_LEAF_FLAG) ? 0u : P.depth[rref];
    const uint32_t d = 1u + (dl > dr ? dl : dr);
    P.depth[node] = d;
    if (A.dp_cost)
        dp_node(A, node, lref, rref, l6, r6, u);
    // the merged cluster takes position i
    P.ref[P.cur][i] = node;
#pragma unroll
    for (int c = 0; c < 6; ++c)
        P.box[P.cur][6ull * i + c] = u[c];
    P.valid[i] = 1u;
    if (P.m == 2u)
        P.counters[1] = d; // the last merge: height of the whole tree
}
__global__ __launch_bounds__(256) void k_ploc_compact(const Ploc P) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.m || !P.valid[i])
        return;
    const uint32_t q = P.pos[i];
    P.ref[P.cur ^ 1][q] = P.ref[P.cur][i];
#pragma unroll
    for (int c = 0; c < 6; ++c)
        P.box[P.cur ^ 1][6ull * q + c] = P.box[P.cur][6ull * i + c];
}
__global__ __launch_bounds__(256) void k_ploc_init(const Ploc P, const BuildArrays A) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n_leaves)
        return;
    P.ref[0][i] = leaf_ref(A, i);
#pragma unroll
    for (int c = 0; c < 6; ++c)
        P.box[0][6ull * i + c] = A.leaf_box[6ull * i + c];
}

} // namespace

namespace rt {

hipError_t ploc_build(uint32_t ploc_radius, const BuildFields &fields, ScratchArena &tmp, hipStream_t stream, PlocTree *out, const char **err) {
    *out = PlocTree{};
    const BuildArrays A{fields};
    const uint32_t n_leaves = A.n_leaves;
    Ploc P{};
    // search radius: 8 positions to either side measured best on both bench scenes (S-sponza / S-10M, wide tree collapsed from
    // it: radius 2: 452 / 217 Msamples/s, 4: 495 / 224, 6: 502 / 224, 8: 496 / 244, 16: 464 / 228, 32: 465 / 231; profiles/r03_wide.txt)
    int radius = 8;
    if (ploc_radius)
        radius = std::min(PLOC_MAX_RADIUS, std::max(1, (int)ploc_radius));
    P.radius = radius;
    for (int k = 0; k < 2; ++k) {
        HIP_TRY_ERR(tmp.alloc(&P.ref[k], (size_t)n_leaves));
        HIP_TRY_ERR(tmp.alloc(&P.box[k], 6ull * n_leaves));
    }
    HIP_TRY_ERR(tmp.alloc(&P.nn, (size_t)n_leaves));
    HIP_TRY_ERR(tmp.alloc(&P.valid, (size_t)n_leaves));
    HIP_TRY_ERR(tmp.alloc(&P.pos, (size_t)n_leaves));
    HIP_TRY_ERR(tmp.alloc(&P.depth, (size_t)n_leaves));
    HIP_TRY_ERR(tmp.alloc(&P.counters, (size_t)4));
    HIP_TRY_ERR(hipMemsetAsync(P.counters, 0, 4 * sizeof(uint32_t), stream));
    ExclusiveScan scan;
    HIP_TRY_ERR(scan.prepare(tmp, P.valid, P.pos, (size_t)n_leaves, stream));
    HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_ploc_init, dim3((n_leaves + 255u) / 256u), dim3(256), 0, stream, P, A)); // one thread per leaf (not grid-stride)
    P.m = n_leaves;
    P.cur = 0;
    while (P.m > 1) {
        const dim3 grid((P.m + 255u) / 256u);
        HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_ploc_nn, grid, dim3(256), 0, stream, P));
        HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_ploc_merge, grid, dim3(256), 0, stream, P, A));
        HIP_TRY_ERR(scan.run(P.valid, P.pos, (size_t)P.m, stream));
        HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_ploc_compact, grid, dim3(256), 0, stream, P));
        uint64_t survivors;
        HIP_TRY_ERR(scan_total(P.valid, P.pos, (size_t)P.m, stream, &survivors));
        const uint32_t m_new = (uint32_t)survivors; // <= P.m
        P.force = (uint64_t)(P.m - m_new) * 32u < P.m ? 1 : 0; // (next to) no progress — a healthy round merges a quarter of the clusters —: pair neighbours next round
        P.m = m_new;
        P.cur ^= 1;
        if (++out->rounds > 4096) {
            if (err)
                *err = "PLOC did not terminate";
            return hipErrorUnknown;
        }
    }
    uint32_t h_counters[4];
    HIP_TRY_ERR(hipMemcpyAsync(&out->root, P.ref[P.cur], sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY_ERR(read_back(h_counters, P.counters, 4, stream));
    out->n_inner = h_counters[0];
    out->height = h_counters[1];
    return hipSuccess;
}

} // namespace rt
