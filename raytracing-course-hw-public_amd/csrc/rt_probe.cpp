// rt_probe.cpp — the entry points that look INTO a scene (rt_abi.h): closest-hit, surface, light and background probes on the
// scene's own kernels, the dumps of the trees in HBM, and rt_bvh_info's reference-style description of them.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rt_env.h"
#include "rt_scene_impl.h"

namespace {

// One probe round trip on the scene's own (non-blocking) stream, every copy ordered with the kernel: `in` goes up, `launch(d_in, d_out)`
// queues the kernel(s) that fill the device buffers d_out[k] (out[k].bytes each), those with a host destination come back in the order
// of `out`. The block is the call's own and released on every return path: a large probe leaves nothing on the scene.
struct ProbeOut {
    void *host; // nullptr: computed, not wanted
    size_t bytes;
};
template <size_t N, class Launch> int probe_round_trip(rt_scene *s, const char *fn, const float *in, size_t in_bytes, const ProbeOut (&out)[N], Launch launch) {
    HIP_TRY(hipSetDevice(s->device));
    rt::DevBuf<uint8_t> block;
    rt::CallIo io(s->stream, block, false);
    const float *d_in;
    void *d_out[N];
    io.in(&d_in, in, in_bytes);
    for (size_t k = 0; k < N; ++k)
        io.out(&d_out[k], out[k].host, out[k].bytes);
    return io.run([&]() -> int {
        if (hipError_t e = launch(d_in, d_out); e != hipSuccess)
            return rt::fail(RT_ERR_HIP, std::string(fn) + ": " + hipGetErrorString(e));
        return RT_OK;
    });
}

} // namespace

extern "C" int rt_cast_rays(rt_scene *s, const float *rays, uint32_t n, uint32_t *prim_out, float *bct_out) {
    if (s && s->group)
        return rt_cast_rays(rt::group_primary(s->group), rays, n, prim_out, bct_out);
    if (!s || (n && (!rays || !prim_out || !bct_out)))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_cast_rays: null argument");
    if (n == 0)
        return RT_OK;
    if (s->facts.wide_built) // no binary tree in HBM: the probe goes through the renderer's own wide kernel
        return rt_cast_rays_ex(s, rays, n, RT_CAST_EXTEND, prim_out, bct_out, nullptr);
    const ProbeOut out[] = {{prim_out, (size_t)n * 4}, {bct_out, (size_t)n * 12}};
    return probe_round_trip(s, "rt_cast_rays", rays, (size_t)n * 24, out, [&](const float *d_rays, void *const *d) {
        return rt::launch_cast(s->dev, d_rays, n, static_cast<uint32_t *>(d[0]), static_cast<float *>(d[1]), s->stream);
    });
}

extern "C" int rt_cast_rays_ex(rt_scene *s, const float *rays, uint32_t n, uint32_t mode, uint32_t *prim_out, float *bct_out, rt_stats *stats) {
    if (s && s->group)
        return rt_cast_rays_ex(rt::group_primary(s->group), rays, n, mode, prim_out, bct_out, stats);
    if (mode == RT_CAST_PROBE && !(s && s->facts.wide_built)) {
        if (stats)
            std::memset(stats, 0, sizeof(*stats));
        return rt_cast_rays(s, rays, n, prim_out, bct_out);
    }
    if (!s || (n && (!rays || !prim_out || !bct_out)) || mode > RT_CAST_PACKET_GLOBAL)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_cast_rays_ex: bad argument");
    if (stats)
        std::memset(stats, 0, sizeof(*stats));
    if (n == 0)
        return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = s->ensure_wavefront(n, 1, 1); rc != RT_OK)
        return rc;
    WfLaunch W{};
    s->wf_bind(W);
    W.ray_depth = 1;
    W.global_best = (mode == RT_CAST_EXTEND_GLOBAL || mode == RT_CAST_PACKET_GLOBAL) ? 1u : 0u;
    W.stats = stats ? s->d_stats : nullptr;
    const bool packet = mode == RT_CAST_PACKET || mode == RT_CAST_PACKET_GLOBAL;
    const ProbeOut out[] = {{prim_out, (size_t)n * 4}, {bct_out, (size_t)n * 12}};
    const int rc = probe_round_trip(s, "rt_cast_rays_ex", rays, (size_t)n * 24, out, [&](const float *d_rays, void *const *d) {
        hipError_t e = stats ? hipMemsetAsync(s->d_stats, 0, sizeof(DevStats), s->stream) : hipSuccess;
        if (e == hipSuccess)
            e = hipEventRecord(s->ev0, s->stream);
        if (e == hipSuccess)
            e = rt::launch_wavefront_cast(s->dev, W, d_rays, n, packet, stats != nullptr, static_cast<uint32_t *>(d[0]), static_cast<float *>(d[1]), s->stream);
        if (e == hipSuccess)
            e = hipEventRecord(s->ev1, s->stream);
        return e;
    });
    if (rc != RT_OK)
        return rc;
    if (stats) {
        DevStats h{};
        HIP_TRY(hipMemcpy(&h, s->d_stats, sizeof(h), hipMemcpyDeviceToHost)); // the stream is idle: as fill_stats reads them
        rt::traversal_stats(h, stats);
        s->second_visits = h.second_visits;
        stats->casts = n;
        float ms = 0;
        if (hipEventElapsedTime(&ms, s->ev0, s->ev1) == hipSuccess)
            stats->kernel_ms = ms;
    }
    return RT_OK;
}

extern "C" int rt_surface_normals(rt_scene *s, const float *rays, uint32_t n, uint32_t *prim_out, float *t_out, float *normal_out, float *shading_out) {
    if (s && s->group)
        return rt_surface_normals(rt::group_primary(s->group), rays, n, prim_out, t_out, normal_out, shading_out);
    if (!s || (n && (!rays || !prim_out || !t_out)))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_surface_normals: null argument");
    if (s->facts.wide_built)
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_surface_normals: a probe of the binary tree; create the scene without RT_BUILD_WIDE");
    if (n == 0)
        return RT_OK;
    const ProbeOut out[] = {{prim_out, (size_t)n * 4}, {t_out, (size_t)n * 4}, {normal_out, (size_t)n * 12}, {shading_out, (size_t)n * 12}};
    return probe_round_trip(s, "rt_surface_normals", rays, (size_t)n * 24, out, [&](const float *d_rays, void *const *d) {
        return rt::launch_surface_normals(s->dev, d_rays, n, static_cast<uint32_t *>(d[0]), static_cast<float *>(d[1]), static_cast<float *>(d[2]), static_cast<float *>(d[3]), s->stream);
    });
}

extern "C" int rt_light_pdf(rt_scene *s, const float *rays, uint32_t n, float *pdf_out) {
    if (s && s->group)
        return rt_light_pdf(rt::group_primary(s->group), rays, n, pdf_out);
    if (!s || (n && (!rays || !pdf_out)))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_light_pdf: null argument");
    if (n == 0)
        return RT_OK;
    const ProbeOut out[] = {{pdf_out, (size_t)n * 4}};
    return probe_round_trip(s, "rt_light_pdf", rays, (size_t)n * 24, out,
                            [&](const float *d_rays, void *const *d) { return rt::launch_light_pdf(s->dev, d_rays, n, static_cast<float *>(d[0]), s->stream); });
}

extern "C" int rt_bg_at(rt_scene *s, const float *dirs, uint32_t n, float *rgb_out) {
    if (s && s->group)
        return rt_bg_at(rt::group_primary(s->group), dirs, n, rgb_out);
    if (!s || (n && (!dirs || !rgb_out)))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_bg_at: null argument");
    if (n == 0)
        return RT_OK;
    const ProbeOut out[] = {{rgb_out, (size_t)n * 12}};
    return probe_round_trip(s, "rt_bg_at", dirs, (size_t)n * 12, out,
                            [&](const float *d_dirs, void *const *d) { return rt::launch_bg_at(s->dev, d_dirs, n, static_cast<float *>(d[0]), s->stream); });
}

// The two probes of a float environment's distribution (rt_set_environment with RT_ENV_IMPORTANCE): env_pdf / env_sample_xi of rt_dev_env.h
static int check_env_probe(const rt_scene *s, const char *fn, const void *in, uint32_t n, const void *out) {
    if (!s || (n && (!in || !out)))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null argument");
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, std::string(fn) + ": a multi-GPU scene has no float environment");
    if (!s->dev.env.texels || !s->dev.env.marg)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the scene has no environment distribution (rt_set_environment with RT_ENV_IMPORTANCE and a map "
                                                              "that is not all zero)");
    return RT_OK;
}
extern "C" int rt_env_pdf(rt_scene *s, const float *dirs, uint32_t n, float *pdf_out) {
    if (int rc = check_env_probe(s, "rt_env_pdf", dirs, n, pdf_out); rc != RT_OK)
        return rc;
    if (n == 0)
        return RT_OK;
    const ProbeOut out[] = {{pdf_out, (size_t)n * 4}};
    return probe_round_trip(s, "rt_env_pdf", dirs, (size_t)n * 12, out,
                            [&](const float *d_dirs, void *const *d) { return rt::launch_env_pdf(s->dev.env, d_dirs, n, static_cast<float *>(d[0]), s->stream); });
}
extern "C" int rt_env_sample(rt_scene *s, const float *xi4, uint32_t n, float *dirs_out) {
    if (int rc = check_env_probe(s, "rt_env_sample", xi4, n, dirs_out); rc != RT_OK)
        return rc;
    if (n == 0)
        return RT_OK;
    for (size_t k = 0; k < (size_t)n * 4; ++k) // the binary searches rely on it: 1.0 would select the cell behind the last
        if (!(xi4[k] >= 0.0f && xi4[k] < 1.0f))
            return rt::fail(RT_ERR_INVALID_ARG, "rt_env_sample: a uniform outside [0, 1)");
    const ProbeOut out[] = {{dirs_out, (size_t)n * 12}};
    return probe_round_trip(s, "rt_env_sample", xi4, (size_t)n * 16, out,
                            [&](const float *d_xi, void *const *d) { return rt::launch_env_sample(s->dev.env, d_xi, n, static_cast<float *>(d[0]), s->stream); });
}

extern "C" int rt_bvh_device_dump(rt_scene *s, int which, uint32_t *n_inner, uint32_t *n_tris, uint32_t *root, uint32_t *nodes64, uint32_t *tris48) {
    if (!s || which < 0 || which > 1)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_bvh_device_dump: bad argument");
    if (s->group)
        return rt_bvh_device_dump(rt::group_primary(s->group), which, n_inner, n_tris, root, nodes64, tris48);
    if (which == 0 && s->facts.wide_built)
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_bvh_device_dump: the scene BVH is the 8-wide tree (RT_BUILD_WIDE): use rt_bvh_wide_dump");
    const DevBvh &b = which == 0 ? s->dev.scene : s->dev.lights;
    if (n_inner)
        *n_inner = s->facts.dev_n_inner[which];
    if (n_tris)
        *n_tris = b.n_tris;
    if (root)
        *root = b.root;
    HIP_TRY(hipSetDevice(s->device));
    if (nodes64 && s->facts.dev_n_inner[which])
        HIP_TRY(hipMemcpy(nodes64, b.nodes, sizeof(DevNode) * (size_t)s->facts.dev_n_inner[which], hipMemcpyDeviceToHost));
    if (tris48 && b.n_tris)
        HIP_TRY(hipMemcpy(tris48, b.tris, sizeof(DevTri) * (size_t)b.n_tris, hipMemcpyDeviceToHost));
    return RT_OK;
}

static int check_compact_scene(const rt_scene *s, const char *fn) {
    if (!s)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null argument");
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, std::string(fn) + ": a probe of one GPU's tree");
    if (s->facts.wide_built)
        return rt::fail(RT_ERR_UNSUPPORTED, std::string(fn) + ": the scene BVH is the 8-wide tree (RT_BUILD_WIDE), which has no compact records");
    return RT_OK;
}

extern "C" int rt_bvh_compact_dump(rt_scene *s, uint32_t *n_inner, uint32_t *compact32) {
    if (int rc = check_compact_scene(s, "rt_bvh_compact_dump"); rc != RT_OK)
        return rc;
    const uint32_t n = s->dev.scene.compact ? s->facts.dev_n_inner[0] : 0u;
    if (n_inner)
        *n_inner = n;
    HIP_TRY(hipSetDevice(s->device));
    if (compact32 && n)
        HIP_TRY(hipMemcpy(compact32, s->dev.scene.compact, sizeof(DevNodeCompact) * (size_t)n, hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_bvh_patch_plane(rt_scene *s, uint32_t node, uint32_t word, float value) {
    if (int rc = check_compact_scene(s, "rt_bvh_patch_plane"); rc != RT_OK)
        return rc;
    const uint32_t n = s->facts.dev_n_inner[0];
    if (node >= n || word >= 12u || !s->dev.scene.compact)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_bvh_patch_plane: no such plane");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    DevNode *nodes = const_cast<DevNode *>(s->dev.scene.nodes);
    HIP_TRY(hipMemcpy(reinterpret_cast<float *>(nodes + node) + word, &value, sizeof(float), hipMemcpyHostToDevice));
    if (hipError_t e = rt::launch_derive_compact(nodes, n, const_cast<DevNodeCompact *>(s->dev.scene.compact), s->num_cus, s->stream); e != hipSuccess)
        return rt::hip_fail(e, "rt_bvh_patch_plane: compact node records");
    HIP_TRY(hipStreamSynchronize(s->stream));
    ++s->geo_generation; // a camera-relative copy of the old records is stale
    s->rebuilt_bvh = rt::HostBvh{};
    return RT_OK;
}

extern "C" int rt_compact_derive_host(uint32_t *nodes64, uint32_t n_inner, uint32_t *compact32) {
    if (n_inner == 0u)
        return RT_OK;
    if (!nodes64 || !compact32)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_compact_derive_host: null argument");
    std::memset(compact32, 0, sizeof(DevNodeCompact) * (size_t)n_inner);
    for (uint32_t i = 0; i < n_inner; ++i)
        compact_derive_node(nodes64, n_inner, i, compact32);
    return RT_OK;
}

extern "C" int rt_second_visits(const rt_scene *s, uint64_t *count) {
    if (!s || !count)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_second_visits: null argument");
    *count = s->group ? 0u : s->second_visits;
    return RT_OK;
}

extern "C" int rt_bvh_wide_dump(rt_scene *s, uint32_t *n_nodes, uint32_t *n_tris, uint32_t *depth, uint32_t *nodes80, uint32_t *tris48) {
    if (!s)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_bvh_wide_dump: null argument");
    if (s->group)
        return rt_bvh_wide_dump(rt::group_primary(s->group), n_nodes, n_tris, depth, nodes80, tris48);
    if (!s->facts.wide_built)
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_bvh_wide_dump: the scene was not built with RT_BUILD_WIDE");
    const DevBvh &b = s->dev.scene;
    if (n_nodes)
        *n_nodes = b.n_wide;
    if (n_tris)
        *n_tris = b.n_tris;
    if (depth)
        *depth = s->facts.wide_depth;
    HIP_TRY(hipSetDevice(s->device));
    if ((!nodes80 && !tris48) || b.n_wide == 0)
        return RT_OK;
    // What the kernels read is the packed blob (rt_wide_pack.hip): it is copied back and DECODED into the documented 80-byte records, breadth
    // first from the root (child_base / tri_base renumbered in that order; tris48 row k is the k-th triangle record met, its pad word still
    // holding the record's DevTri / DevAttr index). A test that walks the result therefore checks the bytes the traversal fetches.
    std::vector<uint4_pod> blob(b.n_units);
    HIP_TRY(hipMemcpy(blob.data(), b.wide, (size_t)b.n_units * 16u, hipMemcpyDeviceToHost));
    std::vector<uint32_t> queue{0u}; // unit index of each node, in output order
    queue.reserve(b.n_wide);
    uint32_t n_tri_out = 0;
    for (size_t qi = 0; qi < queue.size(); ++qi) {
        const uint32_t u = queue[qi];
        if ((uint64_t)u + RT_WIDE_NODE_UNITS > b.n_units || queue.size() > b.n_wide)
            return rt::fail(RT_ERR_HIP, "rt_bvh_wide_dump: the packed tree is inconsistent (node outside the blob, or more nodes than were built)");
        const uint4_pod h = blob[u];
        WideNode rec;
        std::memset(&rec, 0, sizeof(rec));
        const uint32_t m[3] = {h.z & 0xFFFFFu, ((h.z >> 20) | (h.w << 12)) & 0xFFFFFu, (h.w >> 8) & 0xFFFFFu};
        const uint32_t e4[3] = {(h.y >> 24) & 15u, h.y >> 28, h.w >> 28};
        for (int c = 0; c < 3; ++c) {
            rec.p[c] = (float)((double)b.grid.base[c] + (double)m[c] * (double)b.grid.g);
            rec.e[c] = (uint8_t)((int)e4[c] + b.grid.e_base + 127);
        }
        const uint32_t state = h.y & 0xFFFFFFu;
        uint32_t n_inner = 0, n_tri = 0;
        for (uint32_t sl = 0; sl < 8u; ++sl) {
            const uint32_t code = (state >> (3u * sl)) & 7u;
            if (code == 4u) {
                rec.imask |= (uint8_t)(1u << sl);
                ++n_inner;
            } else {
                rec.tri_mask |= code << (3u * sl);
                n_tri += (uint32_t)__builtin_popcount(code);
            }
        }
        rec.child_base = (uint32_t)queue.size();
        rec.tri_base = n_tri_out;
        std::memcpy(&rec.qlo[0][0], &blob[u + 1], 48);
        for (uint32_t r = 0; r < n_inner; ++r)
            queue.push_back(h.x + RT_WIDE_NODE_UNITS * r);
        const uint32_t tu = h.x + RT_WIDE_NODE_UNITS * n_inner;
        if ((uint64_t)tu + (uint64_t)RT_WIDE_TRI_UNITS * n_tri > b.n_units || (uint64_t)n_tri_out + n_tri > b.n_tris)
            return rt::fail(RT_ERR_HIP, "rt_bvh_wide_dump: the packed tree is inconsistent (triangles outside the blob)");
        if (tris48)
            std::memcpy(tris48 + 12ull * n_tri_out, &blob[tu], 48ull * n_tri);
        n_tri_out += n_tri;
        if (nodes80)
            std::memcpy(nodes80 + 20ull * qi, &rec, sizeof(rec));
    }
    if (queue.size() != b.n_wide || n_tri_out != b.n_tris)
        return rt::fail(RT_ERR_HIP, "rt_bvh_wide_dump: the packed tree does not hold every node / triangle that was built");
    return RT_OK;
}

// A device-built scene BVH has no host copy: rebuild the reference-style description (pre-order nodes with their OWN box,
// bvh.h:157-163) from what is in HBM, once, when a caller asks for it.
static int reconstruct_host_bvh(rt_scene *s) {
    const uint32_t n_inner = s->facts.dev_n_inner[0], n_tris = s->dev.scene.n_tris;
    std::vector<DevNode> nodes(n_inner);
    std::vector<DevTri> tris(n_tris);
    HIP_TRY(hipSetDevice(s->device));
    if (n_inner)
        HIP_TRY(hipMemcpy(nodes.data(), s->dev.scene.nodes, sizeof(DevNode) * (size_t)n_inner, hipMemcpyDeviceToHost));
    if (n_tris)
        HIP_TRY(hipMemcpy(tris.data(), s->dev.scene.tris, sizeof(DevTri) * (size_t)n_tris, hipMemcpyDeviceToHost));
    rt::HostBvh &hb = s->rebuilt_bvh;
    hb.nodes.clear();
    hb.order.resize(n_tris);
    for (uint32_t k = 0; k < n_tris; ++k)
        hb.order[k] = tris[k].prim;
    hb.root = RT_NONE;
    if (s->dev.scene.root == RT_NONE)
        return RT_OK;
    struct Item {
        uint32_t ref, parent, side; // side: 0 root, 1 left, 2 right
        float lo[3], hi[3];
    };
    auto leaf_range = [&](uint32_t ref, uint32_t &b, uint32_t &e) {
        b = ref & RT_LEAF_BEGIN_MASK;
        const uint32_t cnt = RT_LEAF_CNT(ref);
        e = b + cnt;
        if (cnt == 0) // big leaf: walk the per-triangle flags
            for (e = b; e < n_tris && !(tris[e].flags & 1u); ++e) {
            }
        if (cnt == 0 && e < n_tris)
            ++e;
    };
    std::vector<Item> stack;
    Item r{};
    r.ref = s->dev.scene.root;
    r.parent = RT_NONE;
    for (int c = 0; c < 3; ++c) { // the root's own box is stored nowhere: union of its children's (or of its triangles)
        r.lo[c] = INFINITY;
        r.hi[c] = -INFINITY;
    }
    if (r.ref & RT_LEAF_FLAG) {
        uint32_t b, e;
        leaf_range(r.ref, b, e);
        for (uint32_t k = b; k < e; ++k)
            for (int v = 0; v < 3; ++v)
                for (int c = 0; c < 3; ++c) {
                    const float x = v == 0 ? tris[k].a[c] : (v == 1 ? tris[k].a[c] + tris[k].v[c] : tris[k].a[c] + tris[k].u[c]);
                    r.lo[c] = std::min(r.lo[c], x);
                    r.hi[c] = std::max(r.hi[c], x);
                }
    } else {
        const DevNode &nd = nodes[r.ref];
        for (int c = 0; c < 3; ++c) {
            r.lo[c] = std::min(nd.lmin[c], nd.rmin[c]);
            r.hi[c] = std::max(nd.lmax[c], nd.rmax[c]);
        }
    }
    stack.push_back(r);
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        const uint32_t idx = (uint32_t)hb.nodes.size();
        rt::HostNode hn{};
        std::memcpy(hn.lo, it.lo, 12);
        std::memcpy(hn.hi, it.hi, 12);
        hn.left = hn.right = RT_NONE;
        if (it.parent != RT_NONE)
            (it.side == 1 ? hb.nodes[it.parent].left : hb.nodes[it.parent].right) = idx;
        if (it.ref & RT_LEAF_FLAG) {
            leaf_range(it.ref, hn.obj_begin, hn.obj_end);
            hb.nodes.push_back(hn);
            continue;
        }
        hb.nodes.push_back(hn);
        const DevNode &nd = nodes[it.ref];
        Item l{}, rr{};
        l.ref = nd.left, l.parent = idx, l.side = 1;
        rr.ref = nd.right, rr.parent = idx, rr.side = 2;
        std::memcpy(l.lo, nd.lmin, 12);
        std::memcpy(l.hi, nd.lmax, 12);
        std::memcpy(rr.lo, nd.rmin, 12);
        std::memcpy(rr.hi, nd.rmax, 12);
        stack.push_back(rr); // pre-order: left subtree first
        stack.push_back(l);
    }
    hb.root = 0;
    return RT_OK;
}

extern "C" int rt_bvh_info(rt_scene *s, int which, uint32_t *n_nodes, uint32_t *n_objects, uint32_t *root, uint32_t *nodes_out,
                           uint32_t *order_out) {
    if (!s || which < 0 || which > 1)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_bvh_info: bad argument");
    if (s->group)
        return rt_bvh_info(rt::group_primary(s->group), which, n_nodes, n_objects, root, nodes_out, order_out);
    if (which == 0 && s->facts.device_built && s->facts.wide_built)
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_bvh_info: the binary tree of a device-built wide scene is not kept");
    if (which == 0 && s->facts.wide_built && s->refitted)
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_bvh_info: the wide tree was refitted (RT_UPDATE_REFIT): the binary tree it was collapsed from is not kept");
    if (which == 0 && s->facts.device_built && s->rebuilt_bvh.nodes.empty() && s->dev.scene.n_tris)
        if (int rc = reconstruct_host_bvh(s); rc != RT_OK)
            return rc;
    const rt::HostBvh &b = (which == 0 && s->facts.device_built) ? s->rebuilt_bvh : rt::prepared_host_bvh(s, which);
    if (n_nodes)
        *n_nodes = (uint32_t)b.nodes.size();
    if (n_objects)
        *n_objects = (uint32_t)b.order.size();
    if (root)
        *root = b.root;
    if (nodes_out) {
        for (size_t i = 0; i < b.nodes.size(); ++i) {
            const rt::HostNode &nd = b.nodes[i];
            std::memcpy(nodes_out + 10 * i, nd.lo, 12);
            std::memcpy(nodes_out + 10 * i + 3, nd.hi, 12);
            nodes_out[10 * i + 6] = nd.left;
            nodes_out[10 * i + 7] = nd.right;
            nodes_out[10 * i + 8] = nd.obj_begin;
            nodes_out[10 * i + 9] = nd.obj_end;
        }
    }
    if (order_out && !b.order.empty())
        std::memcpy(order_out, b.order.data(), b.order.size() * sizeof(uint32_t));
    return RT_OK;
}
