// rt_rays.cpp — rt_render_rays / rt_render_rays_rgb8 (rt_abi.h): the wavefront pipeline over rays and RNG streams the caller supplies.
//
// The call runs rt_render's own pass loop (rt_render.cpp run_passes): n_rays / G outputs take the place of the pixels and G * K samples per
// output the place of the SPP, in (output tile) x (sample range) passes under wavefront_max_paths. The passes are of the kind
// WfPassKind::rays (rt_kernels.h): only the first stage's source differs (it reads the ray buffer where a camera source asks a camera);
// bounces, fold and resolve are rt_render's own launches, so a camera's own primary rays give rt_render's image bit for bit.
#include <algorithm>
#include <cstring>

#include "rt_scene_impl.h"

static int render_rays_impl(rt_scene *s, const rt_params *p, const rt_ray *rays, uint32_t n_rays, uint32_t rays_per_output, float *out_rgb, uint8_t *rgb8_out,
                            rt_stats *stats, const char *fn) {
    const std::string name(fn);
    if (!s || !p)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": null argument");
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, name + ": a multi-GPU scene renders images only; create the scene on one device");
    if (int rc = rt::check_wavefront_entry(p, fn, "caller rays", RT_FLAG_DEVICE_FB | RT_FLAG_COUNTERS | RT_FLAG_MEGAKERNEL | RT_FLAG_GLOBAL_BEST, true); rc != RT_OK)
        return rc;
    const uint32_t G = rays_per_output ? rays_per_output : 1u, K = p->samples;
    if (n_rays % G != 0)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": n_rays is not a multiple of rays_per_output");
    const uint32_t n_out = n_rays / G;
    if ((uint64_t)G * K >= 0x80000000ull || n_out >= 0x80000000u)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": rays_per_output x samples and n_rays / rays_per_output must stay below 2^31");
    if (stats)
        std::memset(stats, 0, sizeof(*stats));
    if (n_rays == 0)
        return RT_OK;
    if (!rays || (!out_rgb && !rgb8_out))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": null argument");
    rt::CallIo io(s->stream, s->staging, (p->flags & RT_FLAG_DEVICE_FB) != 0);
    if ((p->flags & RT_FLAG_DEVICE_FB) && (reinterpret_cast<uintptr_t>(rays) & 15u) != 0)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": a device ray buffer must be 16-byte aligned");
    const auto wall0 = std::chrono::steady_clock::now();
    if (s->dev.ray_depth == 0) // raytracer.h:630-631, as rt_render
        return RT_OK;
    HIP_TRY(hipSetDevice(s->device));

    const uint32_t spo = G * K; // samples per output: the virtual image's SPP
    const size_t fb_floats = (size_t)n_out * 3;
    const rt_ray *d_rays;
    float *d_fb;
    uint8_t *d_rgb8 = nullptr;
    io.in(&d_rays, rays, (size_t)n_rays * sizeof(rt_ray));
    if (rgb8_out) { // the float outputs behind an rgb8 destination are internal
        io.scratch(&d_fb, fb_floats * sizeof(float));
        io.out(&d_rgb8, rgb8_out, fb_floats);
    } else {
        io.out(&d_fb, out_rgb, fb_floats * sizeof(float));
    }
    if (int rc = rgb8_out ? s->ensure_film() : RT_OK; rc != RT_OK)
        return rc;
    const bool counters = stats && (p->flags & RT_FLAG_COUNTERS);
    rt::PacketPolicy pol; // of this call: rt_render's, measured on camera rays of its image shape, is not disturbed
    auto passes = [&]() -> int {
        WfLaunch W = rt::one_row_launch(s, p, n_out, spo, d_fb, counters);
        const WfRays R{reinterpret_cast<const uint4_pod *>(d_rays), G, K, p->seed};
        if (int rc = rt::run_passes(s, p, pol, W, rt::WfPassKind::rays(R), n_out, spo, stats, fn); rc != RT_OK)
            return rc;
        if (rgb8_out) // film on the device (image.h:49-82) over the outputs
            HIP_TRY(rt::launch_film(d_fb, d_rgb8, n_out, 0, 1, n_out, s->film_table.get(), s->stream));
        return RT_OK;
    };
    if (int rc = rt::timed_call(s, counters, &io, passes); rc != RT_OK)
        return rc;
    if (stats)
        return rt::fill_stats(s, counters, (uint64_t)n_rays * K, wall0, pol.lanes_x100, stats);
    return RT_OK;
}

extern "C" int rt_render_rays(rt_scene *s, const rt_params *p, const rt_ray *rays, uint32_t n_rays, uint32_t rays_per_output, float *out_rgb, rt_stats *stats) {
    if (n_rays && !out_rgb)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_render_rays: null argument");
    return render_rays_impl(s, p, rays, n_rays, rays_per_output, out_rgb, nullptr, stats, "rt_render_rays");
}

extern "C" int rt_render_rays_rgb8(rt_scene *s, const rt_params *p, const rt_ray *rays, uint32_t n_rays, uint32_t rays_per_output, uint8_t *rgb8, rt_stats *stats) {
    if (n_rays && !rgb8)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_render_rays_rgb8: null argument");
    return render_rays_impl(s, p, rays, n_rays, rays_per_output, nullptr, rgb8, stats, "rt_render_rays_rgb8");
}
