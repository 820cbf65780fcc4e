// rt_bvh_collapse.hip — step 6 of the device builder (rt_bvh_device.hip): the binary tree collapsed into the 8-wide tree, on the device.
//
// ---- 6. wide collapse, top down (RT_BUILD_WIDE on the device tree): one thread per wide node of the current level.
// The node's children are the roots its binary subtree was cut into by the dynamic program (same decisions, same left-to-right
// order as wide_build.cpp's `collect`); slots by octant (greedy on centroid . corner direction), boxes quantised floor / ceil on
// the node's power-of-two grid; inner children get consecutive records (one atomic per node), leaf slots consecutive triangle
// records (one atomic per node) copied from the Morton-ordered DevTri / DevAttr arrays of step 3.
#include <hip/hip_runtime.h>

#include "rt_bvh_build.h"
#include "rt_kernels.h"
#include "wide_grid.h"

namespace {

struct WideEmit {
    const DevNode *nodes;               // the binary tree (inner nodes)
    const float *leaf_box;              // [n_leaves][6]
    const unsigned long long *dp_dec;
    const DevTri *tris_in;              // Morton order, one triangle per binary leaf
    const DevAttr *attrs_in;
    WideNode *wide;
    DevTri *tris_out;
    DevAttr *attrs_out;
    const uint2 *queue_in;              // {binary inner node, wide record index}
    uint2 *queue_out;
    uint32_t n_in;
    uint32_t *counters;                 // [0] wide records allocated, [1] triangle records allocated, [2] entries of queue_out
    WideGrid grid;                      // origins are snapped to it, cell exponents clamped to its 4-bit range (wide_grid.h), as in wide_build.cpp
};
__device__ __forceinline__ uint32_t dec_ksplit(unsigned long long d, int j) { return (uint32_t)(d >> (3 * (j - 2))) & 7u; }
__device__ __forceinline__ uint32_t dec_eff(unsigned long long d, int i) { return (uint32_t)(d >> (21 + 3 * (i - 1))) & 7u; }
__device__ __forceinline__ bool dec_as_leaf(unsigned long long d) { return (d >> 42) & 1ull; }

__global__ __launch_bounds__(64) void k_wide_emit(const WideEmit E) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= E.n_in)
        return;
    const uint32_t bnode = E.queue_in[q].x, widx = E.queue_in[q].y;
    // ---- the roots this node's subtree is cut into
    uint32_t kid[8];   // binary ref: inner index, or RT_LEAF_FLAG | ... for a single-triangle leaf
    bool kid_leaf[8];  // becomes a leaf slot (a binary leaf, or an inner node of <= 3 triangles the program chose to keep whole)
    float kbox[8][6];
    int nk = 0;
    {
        uint32_t st_ref[16];
        uint32_t st_i[16];
        float st_box[16][6];
        int sp = 0;
        const DevNode nd = E.nodes[bnode];
        const uint32_t k = dec_ksplit(E.dp_dec[bnode], 8);
        st_ref[sp] = nd.right, st_i[sp] = 8u - k;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            st_box[sp][c] = nd.rmin[c], st_box[sp][3 + c] = nd.rmax[c];
        ++sp;
        st_ref[sp] = nd.left, st_i[sp] = k;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            st_box[sp][c] = nd.lmin[c], st_box[sp][3 + c] = nd.lmax[c];
        ++sp;
        while (sp > 0) {
            --sp;
            const uint32_t m = st_ref[sp], i = st_i[sp];
            float b[6];
#pragma unroll
            for (int c = 0; c < 6; ++c)
                b[c] = st_box[sp][c];
            bool root_here = (m & RT_LEAF_FLAG) != 0u;
            unsigned long long d = 0ull;
            uint32_t j = 1u;
            if (!root_here) {
                d = E.dp_dec[m];
                j = dec_eff(d, (int)i);
                root_here = j == 1u;
            }
            if (root_here) {
                kid[nk] = m;
                kid_leaf[nk] = (m & RT_LEAF_FLAG) != 0u || dec_as_leaf(d);
#pragma unroll
                for (int c = 0; c < 6; ++c)
                    kbox[nk][c] = b[c];
                ++nk;
                continue;
            }
            const DevNode mn = E.nodes[m];
            const uint32_t kk = dec_ksplit(d, (int)j);
            st_ref[sp] = mn.right, st_i[sp] = j - kk;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                st_box[sp][c] = mn.rmin[c], st_box[sp][3 + c] = mn.rmax[c];
            ++sp;
            st_ref[sp] = mn.left, st_i[sp] = kk;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                st_box[sp][c] = mn.lmin[c], st_box[sp][3 + c] = mn.lmax[c];
            ++sp;
        }
    }
    // ---- node box, grid
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int i = 0; i < nk; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = fminf(lo[c], kbox[i][c]);
            hi[c] = fmaxf(hi[c], kbox[i][3 + c]);
        }
    WideNode rec;
    int ecell[3];
    float org[3]; // the node's origin: its lower corner snapped down to the scene's origin grid (what the quantised planes are measured from)
    wide_node_frame(E.grid, lo, hi, org, ecell);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        rec.p[c] = org[c];
        rec.e[c] = (uint8_t)(ecell[c] + 127);
    }
    // ---- slots: greedy on dot(child centre - node centre, corner direction of the slot)
    int child_in[8];
#pragma unroll
    for (int s = 0; s < 8; ++s)
        child_in[s] = -1;
    uint32_t assigned = 0u;
    for (int round = 0; round < nk; ++round) {
        float best = -__builtin_inff();
        int bi = -1, bs = -1;
        for (int i = 0; i < nk; ++i) {
            if (assigned & (1u << i))
                continue;
            float dc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                dc[c] = 0.5f * (kbox[i][c] + kbox[i][3 + c]) - 0.5f * (lo[c] + hi[c]);
            for (int s = 0; s < 8; ++s) {
                if (child_in[s] >= 0)
                    continue;
                const float sc = dc[0] * ((s & 1) ? 1.0f : -1.0f) + dc[1] * ((s & 2) ? 1.0f : -1.0f) + dc[2] * ((s & 4) ? 1.0f : -1.0f);
                if (sc > best) {
                    best = sc;
                    bi = i;
                    bs = s;
                }
            }
        }
        if (bi < 0) { // NaN boxes: any free pairing
            for (int i = 0; i < nk && bi < 0; ++i)
                if (!(assigned & (1u << i)))
                    bi = i;
            for (int s = 0; s < 8 && bs < 0; ++s)
                if (child_in[s] < 0)
                    bs = s;
        }
        child_in[bs] = bi;
        assigned |= 1u << bi;
    }
    // ---- counts, allocation
    uint32_t n_inner = 0, n_tri = 0;
    uint32_t cnt[8];
    for (int s = 0; s < 8; ++s) {
        cnt[s] = 0;
        const int i = child_in[s];
        if (i < 0)
            continue;
        if (!kid_leaf[i])
            ++n_inner;
        else {
            // triangles below: 1 for a binary leaf; an inner node kept whole has 2 or 3 single-triangle leaves below it
            uint32_t n = 1;
            if (!(kid[i] & RT_LEAF_FLAG)) {
                const DevNode a = E.nodes[kid[i]];
                n = 0;
                const uint32_t sub[2] = {a.left, a.right};
                for (int t = 0; t < 2; ++t) {
                    if (sub[t] & RT_LEAF_FLAG)
                        n += 1;
                    else
                        n += 2; // <= 3 triangles in all: an inner grandchild holds exactly two leaves
                }
            }
            cnt[s] = n;
            n_tri += n;
        }
    }
    const uint32_t first_child = n_inner ? atomicAdd(E.counters + 0, n_inner) : 0u;
    const uint32_t tri_base = n_tri ? atomicAdd(E.counters + 1, n_tri) : 0u;
    const uint32_t qbase = n_inner ? atomicAdd(E.counters + 2, n_inner) : 0u;
    rec.imask = 0;
    rec.child_base = first_child;
    rec.tri_base = tri_base;
    rec.tri_mask = 0;
    rec.pad = 0;
    uint32_t r_inner = 0, r_tri = 0;
    for (int s = 0; s < 8; ++s) {
        const int i = child_in[s];
        if (i < 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                rec.qlo[c][s] = 255; // empty slot: inverted box
                rec.qhi[c][s] = 0;
            }
            continue;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
            wide_quantise_axis(org[c], ecell[c], kbox[i][c], kbox[i][3 + c], &rec.qlo[c][s], &rec.qhi[c][s]);
        if (!kid_leaf[i]) {
            rec.imask |= (uint8_t)(1u << s);
            E.queue_out[qbase + r_inner] = make_uint2(kid[i], first_child + r_inner);
            ++r_inner;
        } else {
            // the slot's triangles, left to right
            uint32_t leaves[3];
            uint32_t nl = 0;
            if (kid[i] & RT_LEAF_FLAG) {
                leaves[nl++] = kid[i] & RT_LEAF_BEGIN_MASK;
            } else {
                const DevNode a = E.nodes[kid[i]];
                const uint32_t sub[2] = {a.left, a.right};
                for (int t = 0; t < 2; ++t) {
                    if (sub[t] & RT_LEAF_FLAG) {
                        leaves[nl++] = sub[t] & RT_LEAF_BEGIN_MASK;
                    } else {
                        const DevNode g = E.nodes[sub[t]];
                        leaves[nl++] = g.left & RT_LEAF_BEGIN_MASK;
                        leaves[nl++] = g.right & RT_LEAF_BEGIN_MASK;
                    }
                }
            }
            for (uint32_t t = 0; t < nl && t < RT_WIDE_MAX_LEAF_TRIS; ++t) {
                rec.tri_mask |= 1u << (3 * s + (int)t);
                DevTri tr = E.tris_in[leaves[t]];
                tr.flags = 0;
                E.tris_out[tri_base + r_tri] = tr;
                E.attrs_out[tri_base + r_tri] = E.attrs_in[leaves[t]];
                ++r_tri;
            }
        }
    }
    E.wide[widx] = rec;
}

} // namespace

namespace rt {

hipError_t collapse_wide(const BuildFields &A, uint32_t bin_root, const WideGrid &grid, DevArena &outs, ScratchArena &tmp, hipStream_t stream, WideTree *out,
                         const char **err) {
    *out = WideTree{};
    const uint32_t n = A.n, n_leaves = A.n_leaves;
    uint2 *queue[2];
    uint32_t *counters;
    HIP_TRY_ERR(outs.alloc(&out->nodes, (size_t)n_leaves)); // <= one wide node per binary inner node
    HIP_TRY_ERR(outs.alloc(&out->tris, (size_t)n));
    HIP_TRY_ERR(outs.alloc(&out->attrs, (size_t)n));
    HIP_TRY_ERR(tmp.alloc(&queue[0], (size_t)n_leaves));
    HIP_TRY_ERR(tmp.alloc(&queue[1], (size_t)n_leaves));
    HIP_TRY_ERR(tmp.alloc(&counters, (size_t)4));
    const uint32_t init_counters[4] = {1u, 0u, 0u, 0u}; // record 0 = the root
    const uint2 root_entry = make_uint2(bin_root, 0u);   // the binary root (Karras: node 0; PLOC: the last merge) -> wide record 0
    HIP_TRY_ERR(hipMemcpyAsync(counters, init_counters, sizeof(init_counters), hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipMemcpyAsync(queue[0], &root_entry, sizeof(root_entry), hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipStreamSynchronize(stream));
    WideEmit E{};
    E.grid = grid;
    E.nodes = A.nodes, E.leaf_box = A.leaf_box, E.dp_dec = A.dp_dec, E.tris_in = A.tris, E.attrs_in = A.attrs;
    E.wide = out->nodes, E.tris_out = out->tris, E.attrs_out = out->attrs, E.counters = counters;
    uint32_t level_n = 1;
    int cur = 0;
    while (level_n > 0) {
        ++out->depth;
        E.queue_in = queue[cur], E.queue_out = queue[cur ^ 1], E.n_in = level_n;
        HIP_TRY_ERR(hipMemsetAsync(counters + 2, 0, sizeof(uint32_t), stream));
        HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_wide_emit, dim3((level_n + 63u) / 64u), dim3(64), 0, stream, E));
        uint32_t h_counters[4];
        HIP_TRY_ERR(read_back(h_counters, counters, 4, stream));
        level_n = h_counters[2];
        out->n_wide = h_counters[0];
        if (out->depth > 200u) { // cannot happen (a level always consumes its queue); never spin
            if (err)
                *err = "wide collapse did not terminate";
            return hipErrorUnknown;
        }
        cur ^= 1;
    }
    return hipSuccess;
}

} // namespace rt
