// rt_bvh_build.h — what the three translation units of the device builder share (internal; .hip files only):
//   rt_bvh_device.hip    keys, sort, leaves, the Karras radix tree and its refit; the two entry points, which call the stages below
//   rt_bvh_ploc.hip      the PLOC binary tree                  (rt::ploc_build)
//   rt_bvh_collapse.hip  the top-down 8-wide collapse          (rt::collapse_wide)
// Here: the arrays of one build, the wide collapse's dynamic program (run by whichever kernel completes a binary node: k_refit or k_ploc_merge),
// and the declarations of the two stages.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_build_host.h"
#include "rt_device_types.h"

namespace rt {

struct BuildFields {
    const float *pos, *nrm, *tan, *uv;
    const uint32_t *mat;
    const uint32_t *keys_sorted, *prims_sorted;
    uint32_t n, n_leaves, leaf_tris;
    DevTri *tris;
    DevAttr *attrs;
    DevNode *nodes;
    unsigned long long *leaf_keys;
    float *leaf_box; // [n_leaves][6]
    float *node_box; // [n_leaves - 1][6]
    uint32_t *leaf_parent, *node_parent;
    uint32_t *arrived; // [n_leaves - 1]
    uint32_t *fast_bad; // set to 1 if a coordinate violates the div_exact_fast range (rt_dev_trav.h)
    // wide collapse (RT_BUILD_WIDE on top of the device tree): the dynamic program of wide_build.cpp, filled by k_refit / k_ploc_merge
    float *dp_cost;                // [n_leaves - 1][7]: C(n, i), i = 1..7; null = no collapse wanted
    unsigned long long *dp_dec;    // [n_leaves - 1]: ksplit(j = 2..8) 3 bits each from bit 0, eff(i = 1..7) 3 bits each from bit 21, as_leaf bit 42
    uint32_t *dp_ntris;            // [n_leaves - 1]: triangles below
    float cost_node, cost_tri;
};

// The binary tree PLOC built into A.nodes (with A.dp_* filled if wanted): its root, the rounds it took, the inner nodes it allocated
// (n_leaves - 1 for a complete tree) and the root's height. `ploc_radius`: rt_build_options.ploc_radius, 0 = the default. Needs
// A.n_leaves > 1 and k_leaves done on `stream`; blocking. Scratch comes from the caller's arena and lives as long as that.
struct PlocTree {
    uint32_t root = 0, rounds = 0, n_inner = 0, height = 0;
};
hipError_t ploc_build(uint32_t ploc_radius, const BuildFields &A, ScratchArena &tmp, hipStream_t stream, PlocTree *out, const char **err);

// The 8-wide tree collapsed from the binary tree below `bin_root`, level by level from the root; the host only reads each level's size.
// Nodes and records are allocated in `outs`, the queues in `tmp`. Needs A.dp_dec filled and single-triangle leaves; blocking.
struct WideTree {
    WideNode *nodes = nullptr;
    DevTri *tris = nullptr;
    DevAttr *attrs = nullptr;
    uint32_t n_wide = 0, depth = 0;
};
hipError_t collapse_wide(const BuildFields &A, uint32_t bin_root, const WideGrid &grid, DevArena &outs, ScratchArena &tmp, hipStream_t stream, WideTree *out,
                         const char **err);

} // namespace rt

namespace {

// The kernels' parameter. Its fields are rt::BuildFields, which the host passes between the translation units; the kernels keep this name.
struct BuildArrays : rt::BuildFields {};

__device__ __forceinline__ uint32_t leaf_ref(const BuildArrays &A, uint32_t leaf) {
    const uint32_t k0 = leaf * A.leaf_tris, cnt = min(A.leaf_tris, A.n - k0);
    return RT_LEAF_FLAG | (cnt << 27) | k0;
}

__device__ __forceinline__ float box_area6(const float *b) { // surface area of {lo.xyz, hi.xyz}; 0 for an inverted / NaN box
    const float dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
    return (dx >= 0.0f && dy >= 0.0f && dz >= 0.0f) ? 2.0f * (dx * dy + dy * dz + dz * dx) : 0.0f;
}

// The wide collapse's dynamic program for one binary node (wide_build.cpp step 2; children are complete by construction):
// C(n, i) = cheapest representation of the subtree as at most i roots, i = 1..7, and the decisions that reach it.
__device__ __forceinline__ void dp_node(const BuildArrays &A, uint32_t node, uint32_t lref, uint32_t rref, const float *l6, const float *r6, const float *box) {
    const float INF = __builtin_inff();
    float cl[7], cr[7];
    uint32_t nl = 1u, nr = 1u;
    if (lref & RT_LEAF_FLAG) {
        const float a = box_area6(l6) * A.cost_tri;
#pragma unroll
        for (int i = 0; i < 7; ++i)
            cl[i] = a;
    } else {
#pragma unroll
        for (int i = 0; i < 7; ++i)
            cl[i] = __hip_atomic_load(A.dp_cost + 7ull * lref + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        nl = __hip_atomic_load(A.dp_ntris + lref, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (rref & RT_LEAF_FLAG) {
        const float a = box_area6(r6) * A.cost_tri;
#pragma unroll
        for (int i = 0; i < 7; ++i)
            cr[i] = a;
    } else {
#pragma unroll
        for (int i = 0; i < 7; ++i)
            cr[i] = __hip_atomic_load(A.dp_cost + 7ull * rref + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        nr = __hip_atomic_load(A.dp_ntris + rref, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const float area = box_area6(box);
    const uint32_t nt = nl + nr;
    unsigned long long dec = 0ull;
    float dist[9];
#pragma unroll
    for (int j = 2; j <= 8; ++j) {
        float best = INF;
        int bk = 1;
#pragma unroll
        for (int k = 1; k < j; ++k) {
            if (k > 7 || j - k > 7)
                continue;
            const float c = cl[k - 1] + cr[j - k - 1];
            if (c < best) {
                best = c;
                bk = k;
            }
        }
        dist[j] = best;
        dec |= (unsigned long long)bk << (3 * (j - 2));
    }
    const float c_leaf = nt <= RT_WIDE_MAX_LEAF_TRIS ? area * (float)nt * A.cost_tri : INF;
    const float c_internal = dist[8] + area * A.cost_node;
    if (c_leaf <= c_internal)
        dec |= 1ull << 42;
    float c[7];
    int eff = 1;
    c[0] = fminf(c_leaf, c_internal);
    dec |= 1ull << 21;
#pragma unroll
    for (int i = 2; i <= 7; ++i) {
        if (dist[i] < c[i - 2]) {
            c[i - 1] = dist[i];
            eff = i;
        } else {
            c[i - 1] = c[i - 2];
        }
        dec |= (unsigned long long)eff << (21 + 3 * (i - 1));
    }
#pragma unroll
    for (int i = 0; i < 7; ++i)
        A.dp_cost[7ull * node + i] = c[i];
    A.dp_ntris[node] = nt;
    A.dp_dec[node] = dec;
}

} // namespace
