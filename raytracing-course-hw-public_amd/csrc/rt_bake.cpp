// rt_bake.cpp — rt_bake / rt_bake_rays / rt_lightmap_points (rt_abi.h): irradiance, SH probes and light-map texels on the device.
//
// rt_bake has rt_rays.cpp's shape: validate, stage host points through the scene's ray staging buffer, rt_render's own pass loop
// (rt_render.cpp run_passes) over n_points "pixels" x samples, copy out. The passes are of the kind WfPassKind::bake (rt_kernels.h): only the
// first stage's source (each sample's ray is made from the point, rt_dev_bake.h) and the last stage (wf_resolve_bake folds as the bake's kind
// asks) differ; bounces and wf_fold are rt_render's own launches.
// rt_bake_rays writes the same rays as rt_ray records, so rt_render_rays over them gives the bake's samples bit for bit.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rt_scene_impl.h"

// what both entry points refuse of an rt_bake_desc and of a host point buffer (`fn`: the entry point's name)
static int check_bake(const rt_bake_desc *b, const rt_bake_point *host_points, uint32_t n_points, const std::string &name) {
    if (b->kind != RT_BAKE_IRRADIANCE && b->kind != RT_BAKE_SH9)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": unknown bake kind " + std::to_string(b->kind));
    for (uint32_t r : b->reserved)
        if (r != 0)
            return rt::fail(RT_ERR_INVALID_ARG, name + ": reserved words of rt_bake_desc must be 0");
    if (!std::isfinite(b->offset))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": offset must be finite");
    for (uint32_t j = 0; host_points && j < n_points; ++j)
        if (host_points[j].reserved != 0)
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
    if (int rc = check_bake(bake, device_fb ? nullptr : points, n_points, name); rc != RT_OK)
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
    float *d_out = out;
    const rt_bake_point *d_points = points;
    if (!device_fb) {
        if (int rc = s->ensure_fb(out_floats); rc != RT_OK)
            return rc;
        d_out = s->fb.get();
        if (int rc = s->ensure_rays((size_t)n_points * sizeof(rt_bake_point)); rc != RT_OK)
            return rc;
        d_points = reinterpret_cast<const rt_bake_point *>(s->rays.get());
    }
    const bool counters = stats && (p->flags & RT_FLAG_COUNTERS);
    rt::PacketPolicy pol; // of this call, as rt_render_rays keeps its own
    auto upload = [&]() -> int {
        if (!device_fb) // once per call; the caller's buffer outlives the stream sync below
            HIP_TRY(hipMemcpyAsync(s->rays.get(), points, (size_t)n_points * sizeof(rt_bake_point), hipMemcpyHostToDevice, s->stream));
        return RT_OK;
    };
    auto passes = [&]() -> int {
        WfLaunch W = rt::one_row_launch(s, p, n_points, K, nullptr, counters); // no fb: wf_resolve_bake writes WfBake::out
        const WfBake B{reinterpret_cast<const uint4_pod *>(d_points), bake->kind, bake->first_sample, bake->offset, p->seed, d_out};
        return rt::run_passes(s, p, pol, W, rt::WfPassKind::bake(B), n_points, K, stats, "rt_bake");
    };
    if (int rc = rt::timed_call(s, counters, upload, passes); rc != RT_OK)
        return rc;
    if (!device_fb)
        HIP_TRY(hipMemcpy(out, d_out, out_floats * sizeof(float), hipMemcpyDeviceToHost));
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
    if (int rc = check_bake(bake, device_fb || !n ? nullptr : points, n_points, name); rc != RT_OK)
        return rc;
    if (device_fb && ((reinterpret_cast<uintptr_t>(points) & 15u) != 0 || (reinterpret_cast<uintptr_t>(rays_out) & 15u) != 0))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": device buffers must be 16-byte aligned");
    if (n == 0)
        return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    const rt_bake_point *d_points = points;
    void *d_out = rays_out;
    if (!device_fb) { // the ray staging buffer holds the output records, then the points
        if (int rc = s->ensure_rays((size_t)n * sizeof(rt_ray) + (size_t)n_points * sizeof(rt_bake_point)); rc != RT_OK)
            return rc;
        d_out = s->rays.get();
        d_points = reinterpret_cast<const rt_bake_point *>(s->rays.get() + (size_t)n * sizeof(rt_ray));
    }
    auto queue = [&]() -> int {
        if (!device_fb)
            HIP_TRY(hipMemcpyAsync(const_cast<rt_bake_point *>(d_points), points, (size_t)n_points * sizeof(rt_bake_point), hipMemcpyHostToDevice, s->stream));
        const WfBake B{reinterpret_cast<const uint4_pod *>(d_points), bake->kind, bake->first_sample, bake->offset, seed, nullptr};
        HIP_TRY(rt::launch_bake_rays(B, samples, (uint32_t)n, d_out, s->num_cus, s->stream));
        if (!device_fb)
            HIP_TRY(hipMemcpyAsync(rays_out, d_out, (size_t)n * sizeof(rt_ray), hipMemcpyDeviceToHost, s->stream));
        return RT_OK;
    };
    return rt::queue_and_wait(s, queue);
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
    rt::DevBuf<uint32_t> words; // owner[texels], offs[texels], the count
    rt::DevBuf<uint8_t> scan_temp;
    rt::DevBuf<float> in;       // host arrays: positions, normals, lm_uv
    rt::DevBuf<rt_bake_point> pts;
    rt::DevBuf<uint32_t> tex;
    HIP_TRY(words.reserve(2 * texels + 1));
    HIP_TRY(scan_temp.reserve(std::max<size_t>(scan_bytes, 16)));
    uint32_t *owner = words.get(), *offs = owner + texels, *count = offs + texels;
    const float *d_pos = positions, *d_nrm = normals, *d_uv = lm_uv;
    rt_bake_point *d_pts = points_out;
    uint32_t *d_tex = texels_out;
    const uint32_t cap = (uint32_t)std::min<size_t>(capacity, texels); // no more texels can be owned
    if (!device) {
        HIP_TRY(in.reserve((size_t)n_tris * 24));
        HIP_TRY(pts.reserve(std::max<uint32_t>(cap, 1u)));
        HIP_TRY(tex.reserve(std::max<uint32_t>(cap, 1u)));
        d_pos = in.get(), d_nrm = in.get() + (size_t)n_tris * 9, d_uv = in.get() + (size_t)n_tris * 18;
        d_pts = pts.get(), d_tex = tex.get();
    }
    uint32_t h_count = 0;
    auto queue = [&]() -> int {
        if (!device) {
            HIP_TRY(hipMemcpyAsync(in.get(), positions, (size_t)n_tris * 36, hipMemcpyHostToDevice, s->stream));
            HIP_TRY(hipMemcpyAsync(in.get() + (size_t)n_tris * 9, normals, (size_t)n_tris * 36, hipMemcpyHostToDevice, s->stream));
            HIP_TRY(hipMemcpyAsync(in.get() + (size_t)n_tris * 18, lm_uv, (size_t)n_tris * 24, hipMemcpyHostToDevice, s->stream));
        }
        HIP_TRY(rt::launch_lightmap_points(d_pos, d_nrm, d_uv, n_tris, width, height, owner, offs, scan_temp.get(), scan_bytes, d_pts, d_tex, cap, count, s->num_cus,
                                           s->stream));
        HIP_TRY(hipMemcpyAsync(&h_count, count, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        return RT_OK;
    };
    if (int rc = rt::queue_and_wait(s, queue); rc != RT_OK)
        return rc;
    *n_points = h_count;
    const uint32_t written = std::min(h_count, cap);
    if (!device && written) {
        HIP_TRY(hipMemcpy(points_out, d_pts, (size_t)written * sizeof(rt_bake_point), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(texels_out, d_tex, (size_t)written * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return RT_OK;
}
