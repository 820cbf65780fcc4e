// rt_bake.cpp — rt_bake / rt_bake_rays / rt_lightmap_points (rt_abi.h): irradiance, SH probes and light-map texels on the device.
//
// rt_bake has rt_rays.cpp's shape: validate, declare points and outputs on the call's rt::CallIo, rt_render's own pass loop
// (rt_render.cpp run_passes) over n_points "pixels" x samples, copy out. The passes are of the kind WfPassKind::bake (rt_kernels.h): only the
// first stage's source (each sample's ray is made from the point, rt_dev_bake.h) and the last stage (wf_resolve_bake folds as the bake's kind
// asks) differ; bounces and wf_fold are rt_render's own launches.
// rt_bake_rays writes the same rays as rt_ray records, so rt_render_rays over them gives the bake's samples bit for bit.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rt_scene_impl.h"

// what both entry points refuse of an rt_bake_desc and of a host point buffer (`host_points`: the points can be read here; `name`: the entry point's)
static int check_bake(const rt_bake_desc *b, bool host_points, const rt_bake_point *points, uint32_t n_points, const std::string &name) {
    if (b->kind != RT_BAKE_IRRADIANCE && b->kind != RT_BAKE_SH9)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": unknown bake kind " + std::to_string(b->kind));
    for (uint32_t r : b->reserved)
        if (r != 0)
            return rt::fail(RT_ERR_INVALID_ARG, name + ": reserved words of rt_bake_desc must be 0");
    if (!std::isfinite(b->offset))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": offset must be finite");
    for (uint32_t j = 0; host_points && j < n_points; ++j)
        if (points[j].reserved != 0)
            return rt::fail(RT_ERR_INVALID_ARG, name + ": the reserved word of rt_bake_point must be 0");
    return RT_OK;
}

extern "C" int rt_bake(rt_scene *s, const rt_params *p, const rt_bake_desc *bake, const rt_bake_point *points, uint32_t n_points, float *out, rt_stats *stats) {
    const std::string name("rt_bake");
    if (!s || !p || !bake)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": null argument");
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, name + ": a multi-GPU scene renders images only; create the scene on one device");
    if (int rc = rt::check_wavefront_entry(p, "rt_bake", "bake points", RT_FLAG_DEVICE_FB | RT_FLAG_COUNTERS | RT_FLAG_MEGAKERNEL | RT_FLAG_GLOBAL_BEST, true); rc != RT_OK)
        return rc;
    if (p->samples >= 0x80000000u || n_points >= 0x80000000u)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": samples and n_points must stay below 2^31");
    const bool device_fb = (p->flags & RT_FLAG_DEVICE_FB) != 0;
    if (n_points && (!points || !out))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": null argument");
    if (int rc = check_bake(bake, !device_fb, points, n_points, name); rc != RT_OK)
        return rc;
    if (device_fb && ((reinterpret_cast<uintptr_t>(points) & 15u) != 0 || (reinterpret_cast<uintptr_t>(out) & 3u) != 0))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": a device point buffer must be 16-byte aligned, a device output 4-byte");
    if (stats)
        std::memset(stats, 0, sizeof(*stats));
    if (n_points == 0)
        return RT_OK;
    const auto wall0 = std::chrono::steady_clock::now();
    if (s->dev.ray_depth == 0) // raytracer.h:630-631, as rt_render
        return RT_OK;
    HIP_TRY(hipSetDevice(s->device));

    const uint32_t K = p->samples;
    const size_t out_floats = (size_t)n_points * (bake->kind == RT_BAKE_SH9 ? 27u : 3u);
    rt::CallIo io(s->stream, s->staging, device_fb);
    const rt_bake_point *d_points;
    float *d_out;
    io.in(&d_points, points, (size_t)n_points * sizeof(rt_bake_point));
    io.out(&d_out, out, out_floats * sizeof(float));
    const bool counters = stats && (p->flags & RT_FLAG_COUNTERS);
    rt::PacketPolicy pol; // of this call, as rt_render_rays keeps its own
    auto passes = [&]() -> int {
        WfLaunch W = rt::one_row_launch(s, p, n_points, K, nullptr, counters); // no fb: wf_resolve_bake writes WfBake::out
        const WfBake B{reinterpret_cast<const uint4_pod *>(d_points), bake->kind, bake->first_sample, bake->offset, p->seed, d_out};
        return rt::run_passes(s, p, pol, W, rt::WfPassKind::bake(B), n_points, K, stats, "rt_bake");
    };
    if (int rc = rt::timed_call(s, counters, &io, passes); rc != RT_OK)
        return rc;
    if (stats)
        return rt::fill_stats(s, counters, (uint64_t)n_points * K, wall0, pol.lanes_x100, stats);
    return RT_OK;
}

extern "C" int rt_bake_rays(rt_scene *s, const rt_bake_desc *bake, uint64_t seed, const rt_bake_point *points, uint32_t n_points, uint32_t samples, uint32_t flags,
                            rt_ray *rays_out) {
    const std::string name("rt_bake_rays");
    if (!s || !bake)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": null argument");
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, name + ": a multi-GPU scene renders images only; create the scene on one device");
    if (flags & ~(uint32_t)RT_FLAG_DEVICE_FB)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": flags other than RT_FLAG_DEVICE_FB");
    const uint64_t n = (uint64_t)n_points * samples;
    if (n >= 0x80000000ull)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": n_points x samples must stay below 2^31");
    const bool device_fb = (flags & RT_FLAG_DEVICE_FB) != 0;
    if (n && (!points || !rays_out))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": null argument");
    if (int rc = check_bake(bake, !device_fb && n, points, n_points, name); rc != RT_OK)
        return rc;
    if (device_fb && ((reinterpret_cast<uintptr_t>(points) & 15u) != 0 || (reinterpret_cast<uintptr_t>(rays_out) & 15u) != 0))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": device buffers must be 16-byte aligned");
    if (n == 0)
        return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    rt::CallIo io(s->stream, s->staging, device_fb);
    const rt_bake_point *d_points;
    rt_ray *d_out;
    io.out(&d_out, rays_out, (size_t)n * sizeof(rt_ray));
    io.in(&d_points, points, (size_t)n_points * sizeof(rt_bake_point));
    return io.run([&]() -> int {
        const WfBake B{reinterpret_cast<const uint4_pod *>(d_points), bake->kind, bake->first_sample, bake->offset, seed, nullptr};
        HIP_TRY(rt::launch_bake_rays(B, samples, (uint32_t)n, d_out, s->num_cus, s->stream));
        return RT_OK;
    });
}

extern "C" int rt_lightmap_points(rt_scene *s, const float *positions, const float *normals, const float *lm_uv, uint32_t n_tris, uint32_t width, uint32_t height,
                                  uint32_t flags, rt_bake_point *points_out, uint32_t *texels_out, uint32_t capacity, uint32_t *n_points) {
    const std::string name("rt_lightmap_points");
    if (!s || !n_points)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": null argument");
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, name + ": a multi-GPU scene renders images only; create the scene on one device");
    if (flags & ~(uint32_t)RT_FLAG_DEVICE_FB)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": flags other than RT_FLAG_DEVICE_FB");
    if (width == 0 || height == 0 || (uint64_t)width * height >= 0x80000000ull)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": atlas size " + std::to_string(width) + "x" + std::to_string(height));
    if ((n_tris && (!positions || !normals || !lm_uv)) || (capacity && (!points_out || !texels_out)))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": null argument");
    const bool device = (flags & RT_FLAG_DEVICE_FB) != 0;
    auto misaligned = [](const void *q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) != 0; };
    if (device && (misaligned(positions, 4) || misaligned(normals, 4) || misaligned(lm_uv, 4) || misaligned(texels_out, 4) || misaligned(points_out, 16)))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": device arrays must be 4-byte aligned, points_out 16-byte");
    *n_points = 0;
    if (n_tris == 0)
        return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    const size_t texels = (size_t)width * height;
    const size_t scan_bytes = rt::lightmap_scan_temp_bytes(texels);
    const uint32_t cap = (uint32_t)std::min<size_t>(capacity, texels); // no more texels can be owned
    rt::DevBuf<uint8_t> block; // of this call: an atlas's workspace does not stay with the scene
    rt::CallIo io(s->stream, block, device);
    uint32_t *owner, *offs, *count, *d_tex;
    uint8_t *scan_temp;
    const float *d_pos, *d_nrm, *d_uv;
    rt_bake_point *d_pts;
    io.scratch(&owner, texels * 4);
    io.scratch(&offs, texels * 4);
    io.scratch(&count, 4);
    io.scratch(&scan_temp, std::max<size_t>(scan_bytes, 16));
    io.in(&d_pos, positions, (size_t)n_tris * 36);
    io.in(&d_nrm, normals, (size_t)n_tris * 36);
    io.in(&d_uv, lm_uv, (size_t)n_tris * 24);
    const size_t pts = io.out_ranges(&d_pts, points_out, (size_t)cap * sizeof(rt_bake_point)), tex = io.out_ranges(&d_tex, texels_out, (size_t)cap * 4);
    uint32_t h_count = 0;
    auto find = [&]() -> int {
        HIP_TRY(rt::launch_lightmap_points(d_pos, d_nrm, d_uv, n_tris, width, height, owner, offs, scan_temp, scan_bytes, d_pts, d_tex, cap, count, s->num_cus, s->stream));
        HIP_TRY(hipMemcpyAsync(&h_count, count, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        return RT_OK;
    };
    if (int rc = io.run(find); rc != RT_OK)
        return rc;
    *n_points = h_count;
    const uint32_t written = std::min(h_count, cap); // only the records found come back
    io.range(pts, 0, (size_t)written * sizeof(rt_bake_point));
    io.range(tex, 0, (size_t)written * 4);
    return rt::queue_and_wait(s->stream, [&] { return io.download(); });
}
