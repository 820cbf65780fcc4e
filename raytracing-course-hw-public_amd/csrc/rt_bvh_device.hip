// rt_bvh_device.hip — BVH construction ON THE GPU: the production builder for big scenes.
//
// The reference builds its BVH on one host thread with a full std::sort per node and a surface-area sweep
// (src/bvh.h:268-313, 323-366): O(n log^2 n), about half a second per 2*10^5 triangles and minutes at 10^7. The host
// builder of bvh_build.cpp reproduces that topology bit for bit (needed for the parity contract: event counters and exact
// ties follow the tree) and stays the default. This file is the other mode (rt_scene_desc.build_flags &
// RT_BUILD_DEVICE_LBVH): a linear BVH built entirely on the device in a few tens of milliseconds for 10^7 triangles,
// written straight into the SAME HBM layout the traversal kernels read (DevNode: both children's boxes + child refs,
// DevTri in leaf order, DevAttr in the same order), so nothing downstream changes.
//
//   1. scene bounds              block reduction + ordered-integer atomics
//   2. 30-bit Morton code of every triangle's centre (triangle::center, geometry.h:485-487), radix sort (rocPRIM)
//   3. leaves = runs of LEAF consecutive sorted triangles (default 1; the reference's leaves hold 3.9 on average,
//      bvh.h:343-346); per leaf: DevTri / DevAttr records in sorted order, exact AABB of its vertices, 64-bit key = Morton
//      of its first triangle : leaf index (unique, sorted)
//   4. Karras 2012 radix tree over the leaf keys: every inner node finds its own range and split independently
//   5. bottom-up refit: each leaf walks to the root; the second thread to arrive at a node has both child boxes, writes
//      them into that node's DevNode and carries the union upwards (one agent-scope fence + atomic per hand-off)
//   4b / 5b. PLOC instead of 4 and 5, the default: rt_bvh_ploc.hip
//   6. the 8-wide collapse of either binary tree (RT_BUILD_WIDE): rt_bvh_collapse.hip
// This file has steps 2 to 5, rocPRIM's sort and the two entry points, which call the two stages; rt_bvh_build.h is what the three share.
//
// Boxes are exact (min / max of vertex coordinates, no arithmetic), so the traversal's exactness argument
// (div_exact_fast preconditions, rt_dev_trav.h) holds unchanged. What changes is the TOPOLOGY: rays still find the
// closest hit (same t, bit for bit; tests/test_gpu_bvh_device.py), but equal-t ties may resolve to another triangle
// and the event counters differ from the reference's, so this mode is not the parity mode.
#include <hip/hip_runtime.h>

#include <chrono>
#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "rt_bvh_device.h"
#include "rt_build_dev.h"
#include "rt_bvh_build.h"
#include "wide_grid.h"
#include "rt_kernels.h"

namespace {

// Triangles per leaf. Measured (profiles/r02_lbvh.txt): 1 renders fastest at both scene sizes
// (262 k triangles: 83 ms against 107 ms on the reference's tree; 10^7: 166 against 141 ms), 2 and 4 are slower (loose leaf
// boxes along the Morton curve), so the default is one triangle per leaf; rt_build_options.lbvh_leaf_tris (1..8) overrides it for experiments.
constexpr uint32_t LEAF_TRIS_DEFAULT = 1;

__device__ __forceinline__ uint32_t spread10(uint32_t v) { // 10 bits -> every third bit
    v &= 1023u;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// ---- 2. Morton keys of triangle centres
__global__ __launch_bounds__(256) void k_keys(const float *__restrict__ pos, uint32_t n, const uint32_t *bounds, uint32_t *keys, uint32_t *vals) {
    const float lo[3] = {dec_f(bounds[0]), dec_f(bounds[1]), dec_f(bounds[2])};
    float inv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float ext = dec_f(bounds[3 + c]) - lo[c];
        inv[c] = ext > 0.0f ? 1024.0f / ext : 0.0f;
    }
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float *p = pos + 9ull * i;
        uint32_t q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float ctr = (p[c] + p[3 + c] + p[6 + c]) / 3.0f;
            q[c] = (uint32_t)fminf(fmaxf((ctr - lo[c]) * inv[c], 0.0f), 1023.0f); // NaN -> 0
        }
        keys[i] = spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2);
        vals[i] = i;
    }
}

// ---- 3. leaves: records in sorted order, exact boxes, keys
__global__ __launch_bounds__(256) void k_leaves(const BuildArrays A) {
    for (uint32_t leaf = blockIdx.x * blockDim.x + threadIdx.x; leaf < A.n_leaves; leaf += gridDim.x * blockDim.x) {
        const uint32_t k0 = leaf * A.leaf_tris, k1 = min(k0 + A.leaf_tris, A.n);
        float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        bool ok = true;
        for (uint32_t k = k0; k < k1; ++k) {
            DevTri t;
            DevAttr at;
            tri_records(A.pos, A.nrm, A.tan, A.uv, A.mat, A.prims_sorted[k], t, at, lo, hi, ok);
            t.flags = (k == k1 - 1 ? 1u : 0u) | (k == k0 ? 2u : 0u);
            A.tris[k] = t;
            A.attrs[k] = at;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            A.leaf_box[6ull * leaf + c] = lo[c];
            A.leaf_box[6ull * leaf + 3 + c] = hi[c];
        }
        A.leaf_keys[leaf] = ((unsigned long long)A.keys_sorted[k0] << 32) | (unsigned long long)leaf;
        if (!ok)
            *A.fast_bad = 1u;
    }
}

// ---- 4. Karras 2012: inner node i of the radix tree over the sorted, unique leaf keys
__device__ __forceinline__ int delta(const unsigned long long *keys, int n, int i, int j) {
    if (j < 0 || j >= n)
        return -1;
    return __clzll((long long)(keys[i] ^ keys[j]));
}
__global__ __launch_bounds__(256) void k_radix_tree(const BuildArrays A) {
    const int n = (int)A.n_leaves;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n - 1; i += gridDim.x * blockDim.x) {
        const unsigned long long *keys = A.leaf_keys;
        const int d = delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1) >= 0 ? 1 : -1;
        const int dmin = delta(keys, n, i, i - d);
        int lmax = 2;
        while (delta(keys, n, i, i + lmax * d) > dmin)
            lmax *= 2;
        int l = 0;
        for (int t = lmax / 2; t >= 1; t /= 2)
            if (delta(keys, n, i, i + (l + t) * d) > dmin)
                l += t;
        const int j = i + l * d;
        const int dnode = delta(keys, n, i, j);
        int s = 0;
        for (int t = (l + 1) / 2;; t = (t + 1) / 2) {
            if (delta(keys, n, i, i + (s + t) * d) > dnode)
                s += t;
            if (t <= 1)
                break;
        }
        const int gamma = i + s * d + (d < 0 ? -1 : 0);
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        DevNode &nd = A.nodes[i];
        if (lo == gamma) {
            nd.left = leaf_ref(A, (uint32_t)gamma);
            A.leaf_parent[gamma] = (uint32_t)i;
        } else {
            nd.left = (uint32_t)gamma;
            A.node_parent[gamma] = (uint32_t)i;
        }
        if (hi == gamma + 1) {
            nd.right = leaf_ref(A, (uint32_t)(gamma + 1));
            A.leaf_parent[gamma + 1] = (uint32_t)i;
        } else {
            nd.right = (uint32_t)(gamma + 1);
            A.node_parent[gamma + 1] = (uint32_t)i;
        }
        nd.sel = nd.pad = 0;
        if (i == 0)
            A.node_parent[0] = RT_NONE;
    }
}

// ---- 5. refit: the second arrival at a node owns it. Hand-off between workgroups: the first arrival has stored its
// subtree's box, fenced (agent-scope release) and bumped the counter; the second one sees counter == 1, fences
// (agent-scope acquire) and reads that box (MI355X_MICROARCH.md, inter-workgroup visibility).
__global__ __launch_bounds__(256) void k_refit(const BuildArrays A) {
    for (uint32_t leaf = blockIdx.x * blockDim.x + threadIdx.x; leaf < A.n_leaves; leaf += gridDim.x * blockDim.x) {
        float box[6];
#pragma unroll
        for (int c = 0; c < 6; ++c)
            box[c] = A.leaf_box[6ull * leaf + c];
        uint32_t child_is_leaf = 1u, child = leaf;
        uint32_t node = A.leaf_parent[leaf];
        while (node != RT_NONE) {
            // publish this subtree's box where the sibling's thread will look for it
            float *mine = child_is_leaf ? A.leaf_box + 6ull * child : A.node_box + 6ull * child;
            if (!child_is_leaf) {
#pragma unroll
                for (int c = 0; c < 6; ++c)
                    mine[c] = box[c];
            }
            __threadfence();
            const uint32_t before = atomicAdd(A.arrived + node, 1u);
            if (before == 0u)
                break; // first arrival: the sibling's thread will finish this node
            __threadfence();
            DevNode &nd = A.nodes[node];
            const uint32_t lref = nd.left, rref = nd.right;
            const float *lb = (lref & RT_LEAF_FLAG) ? A.leaf_box + 6ull * ((lref & RT_LEAF_BEGIN_MASK) / A.leaf_tris) : A.node_box + 6ull * lref;
            const float *rb = (rref & RT_LEAF_FLAG) ? A.leaf_box + 6ull * ((rref & RT_LEAF_BEGIN_MASK) / A.leaf_tris) : A.node_box + 6ull * rref;
            float l6[6], r6[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                l6[c] = __hip_atomic_load(lb + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                r6[c] = __hip_atomic_load(rb + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                nd.lmin[c] = l6[c];
                nd.lmax[c] = l6[3 + c];
                nd.rmin[c] = r6[c];
                nd.rmax[c] = r6[3 + c];
                box[c] = fminf(l6[c], r6[c]);
                box[3 + c] = fmaxf(l6[3 + c], r6[3 + c]);
            }
            if (A.dp_cost)
                dp_node(A, node, lref, rref, l6, r6, box);
            child_is_leaf = 0u;
            child = node;
            node = A.node_parent[node];
        }
    }
}

} // namespace

namespace rt {

hipError_t build_bvh_device(const rt_scene_desc *d, hipStream_t stream, DeviceBvh *out, const char **err, bool wide, float cost_node, float cost_tri) {
    const uint32_t n = d->n_triangles;
    *out = DeviceBvh{};
    out->root = RT_NONE;
    out->fast_ok = true;
    if (n == 0)
        return hipSuccess;
    // ---- obtain the five device arrays: this entry point uploads them ...
    const auto t0 = std::chrono::steady_clock::now();
    ScratchArena tmp{stream}; // the uploaded arrays: drained, then freed, on every return path
    float *pos, *nrm, *tan, *uv;
    uint32_t *mat;
    HIP_TRY_ERR(tmp.alloc(&pos, 9ull * n));
    HIP_TRY_ERR(tmp.alloc(&nrm, 9ull * n));
    HIP_TRY_ERR(tmp.alloc(&tan, 9ull * n));
    HIP_TRY_ERR(tmp.alloc(&uv, 6ull * n));
    HIP_TRY_ERR(tmp.alloc(&mat, (size_t)n));
    HIP_TRY_ERR(hipMemcpyAsync(pos, d->positions, 36ull * n, hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipMemcpyAsync(nrm, d->normals, 36ull * n, hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipMemcpyAsync(tan, d->tangents, 36ull * n, hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipMemcpyAsync(uv, d->texcoords, 24ull * n, hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipMemcpyAsync(mat, d->material_ids, 4ull * n, hipMemcpyHostToDevice, stream));
    HIP_TRY_ERR(hipStreamSynchronize(stream)); // uploads done = start of the device build proper
    const auto t1 = std::chrono::steady_clock::now();
    // ---- ... and builds from them
    DeviceArrays in;
    in.pos = pos, in.nrm = nrm, in.uv = uv, in.tan = tan, in.mat = mat, in.n = n;
    const hipError_t e = build_bvh_device_arrays(in, d->build, stream, out, err, wide, cost_node, cost_tri);
    if (e == hipSuccess)
        out->upload_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    return e;
}

hipError_t build_bvh_device_arrays(const DeviceArrays &in, const rt_build_options &opt, hipStream_t stream, DeviceBvh *out, const char **err, bool wide, float cost_node,
                                   float cost_tri) {
    const uint32_t n = in.n;
    *out = DeviceBvh{};
    out->root = RT_NONE;
    out->fast_ok = true;
    if (n == 0)
        return hipSuccess;
    ScratchArena tmp{stream}; // scratch of the build and of its stages: drained, then freed, on every return path
    // ---- options
    uint32_t leaf_tris = LEAF_TRIS_DEFAULT;
    if (opt.lbvh_leaf_tris)
        leaf_tris = std::min(8u, std::max(1u, opt.lbvh_leaf_tris));
    // the wide collapse regroups single-triangle leaves itself; scenes of a handful of triangles take the host collapse (rt_scene.cpp)
    wide = wide && n > 8u;
    if (wide)
        leaf_tris = 1;
    const uint32_t n_leaves = (n + leaf_tris - 1) / leaf_tris;

    // ---- keys and sort
    uint32_t *keys[2], *vals[2], *bounds;
    for (int k = 0; k < 2; ++k) {
        HIP_TRY_ERR(tmp.alloc(&keys[k], (size_t)n));
        HIP_TRY_ERR(tmp.alloc(&vals[k], (size_t)n));
    }
    HIP_TRY_ERR(tmp.alloc(&bounds, (size_t)8));
    static const uint32_t init_bounds[8] = {RT_BOUNDS_WORDS_INIT, 0u, 0u}; // [6]: fast_bad
    HIP_TRY_ERR(hipMemcpyAsync(bounds, init_bounds, sizeof(init_bounds), hipMemcpyHostToDevice, stream));
    const auto t1 = std::chrono::steady_clock::now();

    const int blocks = (int)std::min<uint64_t>(((uint64_t)n + 255) / 256, 256u * 16u);
    HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_bounds, dim3(blocks), dim3(256), 0, stream, in.pos, n, bounds));
    HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_keys, dim3(blocks), dim3(256), 0, stream, in.pos, n, bounds, keys[0], vals[0]));
    size_t sort_bytes = 0;
    HIP_TRY_ERR(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys[0], keys[1], vals[0], vals[1], (size_t)n, 0u, 30u, stream));
    char *sort_tmp;
    HIP_TRY_ERR(tmp.alloc(&sort_tmp, sort_bytes));
    HIP_TRY_ERR(rocprim::radix_sort_pairs(sort_tmp, sort_bytes, keys[0], keys[1], vals[0], vals[1], (size_t)n, 0u, 30u, stream));

    // ---- leaves
    // outputs: out->mem owns them, so a failure below leaves nothing behind once the caller lets `out` go. For the wide tree the binary
    // tree and the Morton-ordered records are scaffolding, freed with the scratch: only the wide tree stays.
    DevArena &outs = out->mem, &bin = wide ? tmp : out->mem;
    BuildArrays A{};
    A.pos = in.pos, A.nrm = in.nrm, A.tan = in.tan, A.uv = in.uv, A.mat = in.mat;
    A.keys_sorted = keys[1], A.prims_sorted = vals[1];
    A.n = n, A.n_leaves = n_leaves, A.leaf_tris = leaf_tris;
    HIP_TRY_ERR(bin.alloc(&A.tris, (size_t)n));
    HIP_TRY_ERR(bin.alloc(&A.attrs, (size_t)n));
    HIP_TRY_ERR(bin.alloc(&A.nodes, (size_t)(n_leaves > 1 ? n_leaves - 1 : 1)));
    HIP_TRY_ERR(tmp.alloc(&A.leaf_keys, (size_t)n_leaves));
    HIP_TRY_ERR(tmp.alloc(&A.leaf_box, 6ull * n_leaves));
    HIP_TRY_ERR(tmp.alloc(&A.node_box, 6ull * n_leaves));
    HIP_TRY_ERR(tmp.alloc(&A.leaf_parent, (size_t)n_leaves));
    HIP_TRY_ERR(tmp.alloc(&A.node_parent, (size_t)n_leaves));
    HIP_TRY_ERR(tmp.alloc(&A.arrived, (size_t)n_leaves));
    A.fast_bad = bounds + 6;
    A.cost_node = cost_node, A.cost_tri = cost_tri;
    if (wide) {
        HIP_TRY_ERR(tmp.alloc(&A.dp_cost, 7ull * n_leaves));
        HIP_TRY_ERR(tmp.alloc(&A.dp_dec, (size_t)n_leaves));
        HIP_TRY_ERR(tmp.alloc(&A.dp_ntris, (size_t)n_leaves));
    }
    HIP_TRY_ERR(hipMemsetAsync(A.arrived, 0, 4ull * n_leaves, stream));
    HIP_TRY_ERR(hipMemsetAsync(A.leaf_parent, 0xFF, 4ull * n_leaves, stream)); // RT_NONE: a single leaf has no parent
    const int lblocks = (int)std::min<uint64_t>(((uint64_t)n_leaves + 255) / 256, 256u * 16u);
    HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_leaves, dim3(lblocks), dim3(256), 0, stream, A));

    // ---- binary tree over the leaves: PLOC (default) or the Karras radix tree + refit (rt_build_options.device_builder = RT_BUILDER_LBVH; also the fallback when
    // a PLOC tree comes out deeper than the traversal stacks allow)
    uint32_t bin_root = 0u;
    bool use_ploc = n_leaves > 1 && opt.device_builder != RT_BUILDER_LBVH;
    if (use_ploc) {
        PlocTree ploc;
        const hipError_t e = ploc_build(opt.ploc_radius, A, tmp, stream, &ploc, err);
        if (e != hipSuccess)
            return e;
        bin_root = ploc.root;
        out->rounds = ploc.rounds;
        if (ploc.n_inner != n_leaves - 1u || ploc.height > 60u) // deeper than the traversal stacks (RT_MAX_STACK 64): take the depth-bounded radix tree
            use_ploc = false;
    }
    if (n_leaves > 1 && !use_ploc) {
        HIP_TRY_ERR(hipMemsetAsync(A.arrived, 0, 4ull * n_leaves, stream));
        HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_radix_tree, dim3(lblocks), dim3(256), 0, stream, A));
        HIP_TRY_ERR(RT_LAUNCH_CHECKED(k_refit, dim3(lblocks), dim3(256), 0, stream, A));
        bin_root = 0u;
    }
    out->ploc = use_ploc;

    // ---- bounds read-back
    uint32_t h_bounds[8];
    HIP_TRY_ERR(read_back(h_bounds, bounds, 8, stream));
    const auto t2 = std::chrono::steady_clock::now();
    bounds_decode(h_bounds, out->lo, out->hi);

    // ---- wide collapse on the device
    WideTree w;
    if (wide) {
        out->wide_grid = make_wide_grid(out->lo, out->hi);
        const hipError_t e = collapse_wide(A, bin_root, out->wide_grid, outs, tmp, stream, &w, err);
        if (e != hipSuccess)
            return e;
        A.nodes = nullptr; // the binary tree was scaffolding; the records are the wide tree's, in its order
        A.tris = w.tris;
        A.attrs = w.attrs;
    }
    const auto t3 = std::chrono::steady_clock::now();

    out->wide = w.nodes;
    out->n_wide = w.n_wide;
    out->wide_depth = w.depth;
    out->wide_ms = std::chrono::duration<double, std::milli>(t3 - t2).count();
    out->nodes = A.nodes;
    out->tris = A.tris;
    out->attrs = A.attrs;
    out->n_inner = n_leaves > 1 ? n_leaves - 1 : 0;
    out->n_tris = n;
    out->root = n_leaves > 1 ? bin_root : (RT_LEAF_FLAG | (n << 27) | 0u);
    out->fast_ok = h_bounds[6] == 0u;
    out->upload_ms = 0; // the arrays were here already; build_bvh_device adds the time of its uploads
    out->build_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    return hipSuccess;
}

} // namespace rt
