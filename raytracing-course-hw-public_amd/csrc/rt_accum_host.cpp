// rt_accum_host.cpp — the host side of the accumulators (rt_abi.h rt_accum_*; their kernels are rt_accum.hip).
//
// An accumulator owns its per-pixel state (S, E, n, err, the round's target and list, about 64 B per pixel) and one camera record; it
// borrows the scene's stream, its wavefront workspace and its staging block (rt_call_io.h). Every call ends with the stream synchronised, so an
// rt_render on the same scene in between only ever sees an idle workspace, and never touches the accumulator's buffers.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rt_scene_impl.h"

struct rt_accum {
    rt_scene *scene = nullptr;
    uint32_t width = 0, height = 0;
    WfSensor sensor{};            // its camera: rt_accum_create_sensor's, or the pinhole record of {camera, seed} (host copy of d_sensor)
    WfSensor *d_sensor = nullptr; // WfLaunch::sensors of its passes: the one record
    rt::AccumRound R{};
    rt::DevArena owned{16};
    rt::PacketPolicy pkt; // of its own passes, kept apart from rt_render's
    bool features = false; // RT_ACCUM_FEATURES: F holds the four first-hit sums (F.rec is the scene's, bound per fill)
    WfFeat F{};
    rt::DenoiseBufs D{};   // rt_accum_denoise's workspace (64 B per pixel), allocated by its first call
    bool ids = false;      // rt_accum_attach_ids: I holds the per-pixel id tables (I.rec is the scene's, bound per fill)
    WfIds I{};
    rt::DevBuf<uint32_t> matte_set; // rt_accum_resolve_matte's id set on the device
    bool groups = false;   // rt_accum_attach_light_groups: G holds the group sums and the material table (G.rec and G.tag are the scene's, bound per fill)
    WfGroups G{};
    bool has_samples = false; // a call has queued a pass of this accumulator: ids and light groups can no longer be attached
    ~rt_accum() {
        (void)hipSetDevice(scene->device);
        (void)hipStreamSynchronize(scene->stream); // `owned` frees after this body: on this device, behind this synchronise
        if (counted)
            --scene->live_accums;
    }
    bool counted = false; // it is one of scene->live_accums
};

template <class T> static int accum_alloc(rt_accum *a, size_t bytes, T **ptr, const char *fn) {
    if (hipError_t e = a->owned.alloc_bytes(ptr, bytes); e != hipSuccess)
        return rt::hip_fail(e, fn);
    return RT_OK;
}

extern "C" int rt_accum_create(rt_scene *s, uint32_t width, uint32_t height, const rt_camera *camera, uint64_t seed, rt_accum **out) {
    return rt_accum_create_ex(s, width, height, camera, seed, 0u, out);
}

// rt_accum_create_ex ({camera, seed}; `sensor` null) and rt_accum_create_sensor (`sensor`; camera and seed not read)
static int accum_create(rt_scene *s, uint32_t width, uint32_t height, const rt_camera *camera, uint64_t seed, const rt_sensor *sensor, uint32_t accum_flags, rt_accum **out) {
    if (!s || !out)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_create: null argument");
    *out = nullptr;
    if (accum_flags & ~(uint32_t)RT_ACCUM_FEATURES)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_create_ex: unknown accum_flags bit");
    if (width == 0 || height == 0 || (uint64_t)width * height >= 0x7FFFFFFFull)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_create: image size " + std::to_string(width) + "x" + std::to_string(height));
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_accum_create: accumulators run on single-GPU scenes only");
    HIP_TRY(hipSetDevice(s->device));
    auto a = std::make_unique<rt_accum>();
    a->scene = s;
    a->width = width;
    a->height = height;
    if (sensor) {
        if (int rc = rt::check_sensor(*sensor, width, height, "rt_accum_create_sensor"); rc != RT_OK)
            return rc;
        a->sensor = rt::make_sensor(*sensor, width, height);
    } else {
        a->sensor = rt::make_sensor(camera ? *camera : s->cam, seed, width, height);
    }
    const size_t n = (size_t)width * height;
    auto alloc = [&]<class T>(size_t bytes, T **ptr) -> int { return accum_alloc(a.get(), bytes, ptr, "rt_accum_create"); };
    rt::AccumRound &R = a->R;
    R.width = width;
    R.height = height;
    R.scan_temp_bytes = rt::accum_scan_temp_bytes((uint32_t)n);
    int rc;
    if ((rc = alloc(12 * n, &R.sum)) != RT_OK || (rc = alloc(12 * n, &R.even_sum)) != RT_OK || (rc = alloc(4 * n, &R.count)) != RT_OK ||
        (rc = alloc(4 * n, &R.err)) != RT_OK || (rc = alloc(4 * n, &R.target)) != RT_OK || (rc = alloc(8 * n, &R.scan_in)) != RT_OK ||
        (rc = alloc(8 * n, &R.scan)) != RT_OK || (rc = alloc(4 * n, &R.list_pix)) != RT_OK || (rc = alloc(4 * n, &R.list_base)) != RT_OK ||
        (rc = alloc(4 * (n + 1), &R.list_off)) != RT_OK || (rc = alloc(8, &R.totals)) != RT_OK || (rc = alloc(R.scan_temp_bytes, &R.scan_temp)) != RT_OK ||
        (rc = alloc(sizeof(WfSensor), &a->d_sensor)) != RT_OK)
        return rc;
    if (accum_flags & RT_ACCUM_FEATURES) {
        WfFeat &F = a->F;
        if ((rc = alloc(12 * n, &F.albedo_sum)) != RT_OK || (rc = alloc(12 * n, &F.normal_sum)) != RT_OK || (rc = alloc(4 * n, &F.depth_sum)) != RT_OK ||
            (rc = alloc(4 * n, &F.hits)) != RT_OK)
            return rc;
        HIP_TRY(hipMemsetAsync(F.albedo_sum, 0, 12 * n, s->stream)); // +0.0
        HIP_TRY(hipMemsetAsync(F.normal_sum, 0, 12 * n, s->stream));
        HIP_TRY(hipMemsetAsync(F.depth_sum, 0, 4 * n, s->stream));
        HIP_TRY(hipMemsetAsync(F.hits, 0, 4 * n, s->stream));
        a->features = true;
    }
    HIP_TRY(hipMemsetAsync(R.sum, 0, 12 * n, s->stream)); // +0.0
    HIP_TRY(hipMemsetAsync(R.even_sum, 0, 12 * n, s->stream));
    HIP_TRY(hipMemsetAsync(R.count, 0, 4 * n, s->stream));
    HIP_TRY(hipMemsetD32Async(R.err, 0x7F800000 /* +inf: n_p < 2 */, n, s->stream));
    HIP_TRY(hipMemcpyAsync(a->d_sensor, &a->sensor, sizeof(WfSensor), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    a->counted = true;
    ++s->live_accums; // rt_update_geometry refuses the scene while this one lives
    *out = a.release();
    return RT_OK;
}

extern "C" int rt_accum_create_ex(rt_scene *s, uint32_t width, uint32_t height, const rt_camera *camera, uint64_t seed, uint32_t accum_flags, rt_accum **out) {
    return accum_create(s, width, height, camera, seed, nullptr, accum_flags, out);
}

extern "C" int rt_accum_create_sensor(rt_scene *s, uint32_t width, uint32_t height, const rt_sensor *sensor, uint32_t accum_flags, rt_accum **out) {
    if (out)
        *out = nullptr;
    if (!sensor)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_create_sensor: null argument");
    return accum_create(s, width, height, nullptr, 0, sensor, accum_flags, out);
}

extern "C" void rt_accum_destroy(rt_accum *acc) { delete acc; }

static int accum_check(const rt_accum *a, const rt_params *p, const char *fn, bool reads_samples) {
    if (!a || !p)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null argument");
    if (p->width != a->width || p->height != a->height)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": params size " + std::to_string(p->width) + "x" + std::to_string(p->height) +
                                                " differs from the accumulator's " + std::to_string(a->width) + "x" + std::to_string(a->height));
    return rt::check_wavefront_entry(p, fn, "accumulators", ~(uint32_t)RT_FLAG_DEVICE_FB, reads_samples); // every flag but the one that does not apply
}

// rt_accum_render (ad == nullptr: params->samples more samples for every pixel) and rt_accum_render_adaptive. A judge (or the uniform step)
// writes every pixel's target count; `fill` then plans the list of (p, k_p) in pixel order, reads back {entries, samples} and runs the
// wavefront pipeline over it in passes of floor(max_paths / K) entries, K the list's largest k, until every pixel holds its target.
static int accum_run(rt_accum *a, const rt_params *p, const rt_adaptive *ad, uint32_t *rounds_out, rt_stats *stats) {
    rt_scene *s = a->scene;
    const auto wall0 = std::chrono::steady_clock::now();
    if (stats)
        std::memset(stats, 0, sizeof(*stats));
    if (rounds_out)
        *rounds_out = 0;
    if (s->dev.ray_depth == 0) // raytracer.h:630-631, as rt_render
        return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t n_pix = a->width * a->height;
    const bool counters = stats && (p->flags & RT_FLAG_COUNTERS);
    const uint64_t max_paths = rt::wavefront_max_paths(s, p);
    // the largest k of one list: a pass holds at least one whole entry, and a list's sample prefix stays below 2^32 (rt_accum.hip)
    const uint32_t chunk_cap = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(max_paths, 0xFFFFFFFFull / n_pix));
    WfLaunch W{};
    W.width = a->width;
    W.height = a->height;
    W.shard_count = 1;
    W.shard_block = n_pix;
    W.ray_depth = s->dev.ray_depth;
    W.sensors = a->d_sensor;
    W.view_pixels = n_pix;
    W.global_best = (p->flags & RT_FLAG_GLOBAL_BEST) ? 1u : 0u;
    W.stats = counters ? s->d_stats : nullptr;
    uint32_t passes = 0, packet_passes = 0, rounds = 0;
    uint64_t added = 0;
    // rt_accum_render's progress: per pass, of the passes the call will run (every pixel, samples in lists of at most chunk_cap)
    const uint32_t uni_chunk = std::min(ad ? 1u : p->samples, chunk_cap);
    const uint64_t uni_per_pass = std::max<uint64_t>(1, max_paths / uni_chunk);
    const uint32_t uni_passes = ad ? 0u : (uint32_t)(((uint64_t)p->samples + uni_chunk - 1) / uni_chunk * ((n_pix + uni_per_pass - 1) / uni_per_pass));

    auto fill = [&](uint32_t K, bool *any) -> int {
        const uint32_t C = std::min(K, chunk_cap);
        const uint32_t per_pass = (uint32_t)std::min<uint64_t>(n_pix, std::max<uint64_t>(1, max_paths / C));
        for (;;) {
            HIP_TRY(rt::launch_accum_plan(a->R, C, s->stream));
            uint32_t tot[2] = {0u, 0u}; // entries, samples of the list
            HIP_TRY(hipMemcpyAsync(tot, a->R.totals, sizeof(tot), hipMemcpyDeviceToHost, s->stream));
            HIP_TRY(hipStreamSynchronize(s->stream));
            if (tot[0] == 0)
                return RT_OK;
            *any = true;
            const uint64_t cap = std::min<uint64_t>((uint64_t)std::min(per_pass, tot[0]) * C, tot[1]);
            if (int rc = s->ensure_wavefront(cap, std::max<uint64_t>(s->wf_pixels_cap, 1), s->dev.ray_depth); rc != RT_OK)
                return rc;
            if (a->features) {
                if (int rc = s->ensure_features(); rc != RT_OK)
                    return rc;
                a->F.rec = s->wf_feat.get();
            }
            if (a->ids) {
                if (int rc = s->ensure_ids(); rc != RT_OK)
                    return rc;
                a->I.rec = s->wf_ids.get();
            }
            if (a->groups) {
                if (int rc = s->ensure_groups(a->G.n_groups); rc != RT_OK)
                    return rc;
                a->G.rec = s->wf_group_rec.get();
                a->G.tag = s->wf_group_tag.get();
            }
            s->wf_bind(W);
            W.fb = nullptr;
            W.accum = nullptr; // wf_resolve does not run on an accumulator pass
            for (uint32_t e0 = 0; e0 < tot[0]; e0 += per_pass) {
                WfAccum A{a->R.sum, a->R.even_sum, a->R.count, a->R.list_pix, a->R.list_base, a->R.list_off, e0, std::min(per_pass, tot[0] - e0)};
                W.n_paths = (uint32_t)std::min<uint64_t>((uint64_t)A.n_entries * C, tot[1]); // an upper bound: the first stage reads the exact count
                W.first_pixel = 0, W.pass_pixels = A.n_entries;
                W.first_sample = 0, W.pass_samples = C, W.samples = C;
                a->has_samples = true;
                const rt::WfPassKind kind = rt::WfPassKind::list(A, a->features ? &a->F : nullptr, a->ids ? &a->I : nullptr, a->groups ? &a->G : nullptr, a->sensor);
                HIP_TRY(rt::launch_pass(s, p, a->pkt, W, kind, rt::WfPassStep{true, true, stats != nullptr}));
                passes += 1;
                packet_passes += W.use_packet;
                if (p->progress && !ad) {
                    HIP_TRY(hipStreamSynchronize(s->stream));
                    p->progress(passes, std::max(passes, uni_passes), p->progress_user);
                }
            }
            added += tot[1];
        }
    };

    auto rounds_of_call = [&]() -> int {
        if (!ad) {
            HIP_TRY(rt::launch_accum_uniform(a->R, p->samples, s->stream));
            bool any = false;
            if (int rc = fill(p->samples, &any); rc != RT_OK)
                return rc;
        } else {
            const uint32_t mn = ad->min_samples ? ad->min_samples : 16u, st = ad->step ? ad->step : 32u, mx = ad->max_samples; // rt_abi.h rt_adaptive
            const uint32_t bound = 1u + (mx - std::min(mn, mx) + st - 1u) / st; // rounds one pixel can take part in
            for (uint32_t r = 0;; ++r) {
                HIP_TRY(rt::launch_accum_judge(a->R, r == 0 ? 1 : 0, ad->threshold, mn, mx, st, s->stream));
                bool any = false;
                if (int rc = fill(r == 0 ? mn : st, &any); rc != RT_OK)
                    return rc;
                if (any) {
                    ++rounds;
                    if (p->progress)
                        p->progress(rounds, std::max(rounds, bound), p->progress_user);
                } else if (r > 0) {
                    break; // this judge found no active pixel: err is the final state's
                }
            }
        }
        return RT_OK;
    };
    if (int rc = rt::timed_call(s, counters, nullptr, rounds_of_call); rc != RT_OK)
        return rc;
    if (rounds_out)
        *rounds_out = rounds;
    if (stats) {
        if (int rc = rt::fill_stats(s, counters, added, wall0, a->pkt.lanes_x100, stats); rc != RT_OK)
            return rc;
        stats->passes = passes;
        stats->packet_passes = packet_passes;
    }
    return RT_OK;
}

extern "C" int rt_accum_render(rt_accum *acc, const rt_params *params, rt_stats *stats) {
    if (int rc = accum_check(acc, params, "rt_accum_render", true); rc != RT_OK)
        return rc;
    return accum_run(acc, params, nullptr, nullptr, stats);
}

extern "C" int rt_accum_render_adaptive(rt_accum *acc, const rt_params *params, const rt_adaptive *ad, uint32_t *rounds, rt_stats *stats) {
    if (int rc = accum_check(acc, params, "rt_accum_render_adaptive", false); rc != RT_OK)
        return rc;
    if (!ad)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_render_adaptive: null argument");
    if (!(ad->threshold >= 0.0f) || std::isinf(ad->threshold))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_render_adaptive: threshold must be finite and >= 0");
    const uint32_t mn = ad->min_samples ? ad->min_samples : 16u;
    if (mn == 1u || ad->max_samples < mn)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_render_adaptive: min_samples must be 0 or >= 2, and max_samples >= min_samples");
    for (uint32_t r : ad->reserved)
        if (r != 0)
            return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_render_adaptive: reserved fields must be 0");
    return accum_run(acc, params, ad, rounds, stats);
}

extern "C" int rt_accum_resolve(rt_accum *acc, uint32_t flags, float *fb_rgb) {
    if (!acc || !fb_rgb || (flags & ~(uint32_t)RT_FLAG_DEVICE_FB))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_resolve: null argument or flags other than RT_FLAG_DEVICE_FB");
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    rt::CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    float *d_fb;
    io.out(&d_fb, fb_rgb, (size_t)acc->width * acc->height * 12);
    return io.run([&]() -> int {
        HIP_TRY(rt::launch_accum_image(acc->R, d_fb, s->stream));
        return RT_OK;
    });
}

// `image` fills an internal float image; the film (image.h:49-82, as rt_render_rgb8) makes the rgb8 destination of it
template <class Image> static int film_image(rt_accum *acc, uint32_t flags, uint8_t *rgb8, Image image) {
    rt_scene *s = acc->scene;
    if (int rc = s->ensure_film(); rc != RT_OK)
        return rc;
    const uint32_t n = acc->width * acc->height;
    rt::CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    float *d_fb;
    uint8_t *d_rgb8;
    io.scratch(&d_fb, 12ull * n);
    io.out(&d_rgb8, rgb8, 3ull * n);
    return io.run([&]() -> int {
        HIP_TRY(image(d_fb));
        HIP_TRY(rt::launch_film(d_fb, d_rgb8, n, 0, 1, n, s->film_table.get(), s->stream));
        return RT_OK;
    });
}

extern "C" int rt_accum_resolve_rgb8(rt_accum *acc, uint32_t flags, uint8_t *rgb8) {
    if (!acc || !rgb8 || (flags & ~(uint32_t)RT_FLAG_DEVICE_FB))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_resolve_rgb8: null argument or flags other than RT_FLAG_DEVICE_FB");
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    return film_image(acc, flags, rgb8, [&](float *d_fb) { return rt::launch_accum_image(acc->R, d_fb, s->stream); });
}

// the accumulator's own arrays, each to a host destination that is not null
struct ReadBack {
    void *host;
    const void *dev;
    size_t bytes;
};
static int read_back(rt_scene *s, std::initializer_list<ReadBack> list) {
    return rt::queue_and_wait(s->stream, [&]() -> int {
        for (const ReadBack &r : list)
            if (r.host)
                HIP_TRY(hipMemcpyAsync(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost, s->stream));
        return RT_OK;
    });
}

extern "C" int rt_accum_read(rt_accum *acc, float *sum_rgb, float *even_sum_rgb, uint32_t *samples, float *error) {
    if (!acc)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_read: null accumulator");
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)acc->width * acc->height;
    return read_back(s, {{sum_rgb, acc->R.sum, 12 * n}, {even_sum_rgb, acc->R.even_sum, 12 * n}, {samples, acc->R.count, 4 * n}, {error, acc->R.err, 4 * n}});
}

// ---- first-hit features and the denoiser (rt_abi.h RT_ACCUM_FEATURES, rt_accum_denoise)
static int feature_check(const rt_accum *acc, const char *fn) {
    if (!acc)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null accumulator");
    if (!acc->features)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the accumulator was created without RT_ACCUM_FEATURES");
    return RT_OK;
}

extern "C" int rt_accum_read_features(rt_accum *acc, float *albedo_sum, float *normal_sum, float *depth_sum, uint32_t *hits) {
    if (int rc = feature_check(acc, "rt_accum_read_features"); rc != RT_OK)
        return rc;
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)acc->width * acc->height;
    return read_back(s, {{albedo_sum, acc->F.albedo_sum, 12 * n}, {normal_sum, acc->F.normal_sum, 12 * n}, {depth_sum, acc->F.depth_sum, 4 * n}, {hits, acc->F.hits, 4 * n}});
}

extern "C" int rt_accum_resolve_features(rt_accum *acc, uint32_t flags, float *albedo, float *normal, float *depth) {
    if (int rc = feature_check(acc, "rt_accum_resolve_features"); rc != RT_OK)
        return rc;
    if (flags & ~(uint32_t)RT_FLAG_DEVICE_FB)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_resolve_features: flags other than RT_FLAG_DEVICE_FB");
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)acc->width * acc->height;
    rt::CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    float *d_a, *d_n, *d_z; // on a host call all three are computed; a null destination is not copied
    io.out(&d_a, albedo, 12 * n);
    io.out(&d_n, normal, 12 * n);
    io.out(&d_z, depth, 4 * n);
    return io.run([&]() -> int {
        HIP_TRY(rt::launch_accum_feature_means(acc->R, acc->F, d_a, d_n, d_z, s->stream));
        return RT_OK;
    });
}

// the defaults of rt_denoise: chosen by the sweep recorded in profiles/denoise_quality.txt
static int denoise_options(const rt_accum *acc, const rt_denoise *opt, uint32_t flags, const void *out, const char *fn, rt::DenoiseOpt *O) {
    if (int rc = feature_check(acc, fn); rc != RT_OK)
        return rc;
    if (!out || (flags & ~(uint32_t)RT_FLAG_DEVICE_FB))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null buffer or flags other than RT_FLAG_DEVICE_FB");
    const rt_denoise zero{};
    const rt_denoise &o = opt ? *opt : zero;
    for (uint32_t r : o.reserved)
        if (r != 0)
            return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": reserved fields must be 0");
    if (o.iterations > 8u || o.normal_sharpness > 8u || (o.flags & ~(uint32_t)RT_DENOISE_NO_DEMODULATE))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": iterations and normal_sharpness are at most 8; unknown rt_denoise.flags bit");
    if (!(o.sigma_color >= 0.0f) || std::isinf(o.sigma_color) || !(o.sigma_depth >= 0.0f) || std::isinf(o.sigma_depth))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": sigma_color and sigma_depth must be finite and >= 0");
    O->iterations = o.iterations ? o.iterations : 5u;
    O->sigma_color = o.sigma_color != 0.0f ? o.sigma_color : 8.0f;
    O->sigma_depth = o.sigma_depth != 0.0f ? o.sigma_depth : 0.5f;
    O->sharpness = o.normal_sharpness ? o.normal_sharpness : 3u;
    O->demodulate = (o.flags & RT_DENOISE_NO_DEMODULATE) ? 0u : 1u;
    return RT_OK;
}

static int denoise_buffers(rt_accum *acc, const char *fn) {
    if (acc->D.guide)
        return RT_OK;
    const size_t n = (size_t)acc->width * acc->height;
    int rc;
    if ((rc = accum_alloc(acc, 16 * n, &acc->D.sig[0], fn)) != RT_OK || (rc = accum_alloc(acc, 16 * n, &acc->D.sig[1], fn)) != RT_OK ||
        (rc = accum_alloc(acc, 16 * n, &acc->D.den, fn)) != RT_OK)
        return rc;
    return accum_alloc(acc, 32 * n, &acc->D.guide, fn); // last: its pointer says the workspace is complete
}

extern "C" int rt_accum_denoise(rt_accum *acc, const rt_denoise *opt, uint32_t flags, float *fb_rgb) {
    rt::DenoiseOpt O{};
    if (int rc = denoise_options(acc, opt, flags, fb_rgb, "rt_accum_denoise", &O); rc != RT_OK)
        return rc;
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = denoise_buffers(acc, "rt_accum_denoise"); rc != RT_OK)
        return rc;
    rt::CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    float *d_fb;
    io.out(&d_fb, fb_rgb, (size_t)acc->width * acc->height * 12);
    return io.run([&]() -> int {
        HIP_TRY(rt::launch_denoise(acc->R, acc->F, acc->D, O, d_fb, s->stream));
        return RT_OK;
    });
}

extern "C" int rt_accum_denoise_rgb8(rt_accum *acc, const rt_denoise *opt, uint32_t flags, uint8_t *rgb8) {
    rt::DenoiseOpt O{};
    if (int rc = denoise_options(acc, opt, flags, rgb8, "rt_accum_denoise_rgb8", &O); rc != RT_OK)
        return rc;
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = denoise_buffers(acc, "rt_accum_denoise_rgb8"); rc != RT_OK)
        return rc;
    return film_image(acc, flags, rgb8, [&](float *d_fb) { return rt::launch_denoise(acc->R, acc->F, acc->D, O, d_fb, s->stream); });
}

// ---- id mattes (rt_abi.h rt_accum_attach_ids: the rule; the kernels: rt_wavefront.hip wf_ids / wf_resolve_ids, rt_accum.hip)
extern "C" int rt_accum_attach_ids(rt_accum *acc, const rt_id_desc *desc) {
    if (!acc || !desc)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: null argument");
    rt_scene *s = acc->scene;
    const bool user = desc->kind == RT_ID_USER, device_table = (desc->flags & RT_FLAG_DEVICE_FB) != 0;
    if (desc->kind > (uint32_t)RT_ID_USER)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: unknown kind " + std::to_string(desc->kind));
    if (desc->slots > RT_ID_MAX_SLOTS)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: slots must be 0 (= 4) or 1..16");
    if (desc->reserved[0] != 0 || desc->reserved[1] != 0 || (desc->flags & ~(uint32_t)RT_FLAG_DEVICE_FB))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: reserved fields must be 0; flags other than RT_FLAG_DEVICE_FB");
    const uint32_t n_table = s->dev.n_triangles + s->dev.n_prims;
    if (user && (!desc->table || desc->n_table != n_table))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: RT_ID_USER needs a table of n_triangles + n_primitives = " + std::to_string(n_table) + " ids");
    if (!user && (desc->table || desc->n_table != 0))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: only RT_ID_USER takes a table");
    if (user && device_table && (reinterpret_cast<uintptr_t>(desc->table) & 3u))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: the device table must be 4-byte aligned");
    if (acc->ids)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: the accumulator already has ids");
    if (acc->has_samples)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: the accumulator already holds samples; attach ids before the first render");
    HIP_TRY(hipSetDevice(s->device));
    WfIds I{};
    I.kind = desc->kind;
    I.k = desc->slots ? desc->slots : 4u;
    I.pixels = acc->width * acc->height;
    const size_t n = I.pixels, words = n * I.k;
    uint32_t *table = nullptr;
    int rc;
    if ((rc = accum_alloc(acc, 4 * words, &I.slot_id, "rt_accum_attach_ids")) != RT_OK || (rc = accum_alloc(acc, 4 * words, &I.slot_count, "rt_accum_attach_ids")) != RT_OK ||
        (rc = accum_alloc(acc, 4 * n, &I.other, "rt_accum_attach_ids")) != RT_OK ||
        (user && (rc = accum_alloc(acc, 4 * (size_t)n_table, &table, "rt_accum_attach_ids")) != RT_OK))
        return rc; // what was allocated stays with the accumulator's arena, unused, until rt_accum_destroy
    auto queue = [&]() -> int {
        HIP_TRY(hipMemsetAsync(I.slot_id, 0, 4 * words, s->stream));
        HIP_TRY(hipMemsetAsync(I.slot_count, 0, 4 * words, s->stream));
        HIP_TRY(hipMemsetAsync(I.other, 0, 4 * n, s->stream));
        if (user && n_table)
            HIP_TRY(hipMemcpyAsync(table, desc->table, 4 * (size_t)n_table, device_table ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
        return RT_OK;
    };
    if ((rc = rt::queue_and_wait(s->stream, queue)) != RT_OK)
        return rc;
    I.table = table;
    acc->I = I;
    acc->ids = true;
    return RT_OK;
}

static int ids_check(const rt_accum *acc, const char *fn) {
    if (!acc)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null accumulator");
    if (!acc->ids)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the accumulator has no ids (rt_accum_attach_ids)");
    return RT_OK;
}

extern "C" int rt_accum_read_ids(rt_accum *acc, uint32_t *ids, uint32_t *counts, uint32_t *other) {
    if (int rc = ids_check(acc, "rt_accum_read_ids"); rc != RT_OK)
        return rc;
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = acc->I.pixels, K = acc->I.k;
    std::vector<uint32_t> slot_major; // the device keeps slot j of pixel p at j * pixels + p
    for (auto [dst, src] : {std::pair{ids, acc->I.slot_id}, std::pair{counts, acc->I.slot_count}}) {
        if (!dst)
            continue;
        slot_major.resize(n * K);
        if (int rc = read_back(s, {{slot_major.data(), src, 4 * n * K}}); rc != RT_OK)
            return rc;
        for (size_t p = 0; p < n; ++p)
            for (size_t j = 0; j < K; ++j)
                dst[p * K + j] = slot_major[j * n + p];
    }
    return read_back(s, {{other, acc->I.other, 4 * n}});
}

extern "C" int rt_accum_resolve_labels(rt_accum *acc, uint32_t flags, uint32_t *label, float *coverage) {
    if (int rc = ids_check(acc, "rt_accum_resolve_labels"); rc != RT_OK)
        return rc;
    if (flags & ~(uint32_t)RT_FLAG_DEVICE_FB)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_resolve_labels: flags other than RT_FLAG_DEVICE_FB");
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    rt::CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    uint32_t *d_label;
    float *d_cov;
    io.out(&d_label, label, 4 * (size_t)acc->I.pixels);
    io.out(&d_cov, coverage, 4 * (size_t)acc->I.pixels);
    return io.run([&]() -> int {
        HIP_TRY(rt::launch_accum_labels(acc->R, acc->I, d_label, d_cov, s->stream));
        return RT_OK;
    });
}

extern "C" int rt_accum_resolve_matte(rt_accum *acc, uint32_t flags, const uint32_t *ids, uint32_t n_ids, float *matte) {
    if (int rc = ids_check(acc, "rt_accum_resolve_matte"); rc != RT_OK)
        return rc;
    if (!ids || !matte || n_ids == 0 || n_ids > 4096u || (flags & ~(uint32_t)RT_FLAG_DEVICE_FB))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_resolve_matte: null ids or matte, n_ids outside 1..4096, or flags other than RT_FLAG_DEVICE_FB");
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    std::vector<uint32_t> set(ids, ids + n_ids); // sorted, each id once: the kernel's binary search
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    HIP_TRY(acc->matte_set.reserve(set.size()));
    rt::CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    float *d_matte;
    io.out(&d_matte, matte, 4 * (size_t)acc->I.pixels);
    return io.run([&]() -> int { // `set` is a local: nothing of this may be in flight when it dies
        HIP_TRY(hipMemcpyAsync(acc->matte_set.get(), set.data(), 4 * set.size(), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(rt::launch_accum_matte(acc->R, acc->I, acc->matte_set.get(), (uint32_t)set.size(), d_matte, s->stream));
        return RT_OK;
    });
}

// ---- light groups (rt_abi.h rt_accum_attach_light_groups: the rule; the kernels: rt_wavefront.hip wf_group_tags, rt_wf_stages.h wf_fold_groups /
// wf_resolve_groups, rt_accum.hip)
extern "C" int rt_accum_attach_light_groups(rt_accum *acc, const rt_light_group_desc *desc) {
    const char *fn = "rt_accum_attach_light_groups";
    if (!acc || !desc)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null argument");
    rt_scene *s = acc->scene;
    const uint32_t G = desc->n_groups, n_mats = (uint32_t)s->prep->mats.size();
    const bool device_table = (desc->flags & RT_FLAG_DEVICE_FB) != 0;
    auto in_range = [G](uint32_t g) { return g < G || g == RT_LIGHT_GROUP_NONE; };
    if (G == 0 || G > RT_LIGHT_GROUP_MAX)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": n_groups must be 1.." + std::to_string(RT_LIGHT_GROUP_MAX));
    if (desc->reserved[0] != 0 || desc->reserved[1] != 0 || (desc->flags & ~(uint32_t)RT_FLAG_DEVICE_FB))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": reserved fields must be 0; flags other than RT_FLAG_DEVICE_FB");
    if (!desc->material_group || desc->n_materials != n_mats)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": material_group must hold the scene's " + std::to_string(n_mats) + " materials");
    if (device_table && (reinterpret_cast<uintptr_t>(desc->material_group) & 3u))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the device table must be 4-byte aligned");
    if (!in_range(desc->background_group))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": background_group must be below n_groups, or RT_LIGHT_GROUP_NONE");
    if (acc->groups)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the accumulator already has light groups");
    if (acc->has_samples)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the accumulator already holds samples; attach light groups before the first render");
    HIP_TRY(hipSetDevice(s->device));
    std::vector<uint32_t> words(n_mats); // the entries are checked on the host, wherever the table lives
    if (device_table) {
        if (int rc = rt::queue_and_wait(s->stream, [&]() -> int {
                HIP_TRY(hipMemcpyAsync(words.data(), desc->material_group, 4 * (size_t)n_mats, hipMemcpyDeviceToHost, s->stream));
                return RT_OK;
            });
            rc != RT_OK)
            return rc;
    } else {
        std::copy(desc->material_group, desc->material_group + n_mats, words.begin());
    }
    std::vector<uint8_t> bytes(n_mats);
    for (uint32_t m = 0; m < n_mats; ++m) {
        if (!in_range(words[m]))
            return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": material_group[" + std::to_string(m) + "] is neither below n_groups nor RT_LIGHT_GROUP_NONE");
        bytes[m] = words[m] == RT_LIGHT_GROUP_NONE ? (uint8_t)WF_GROUP_NONE : (uint8_t)words[m];
    }
    WfGroups W{};
    W.n_groups = G;
    W.background = desc->background_group == RT_LIGHT_GROUP_NONE ? WF_GROUP_NONE : desc->background_group;
    W.pixels = acc->width * acc->height;
    const size_t sum_bytes = 12 * (size_t)G * W.pixels;
    uint8_t *table = nullptr;
    int rc;
    if ((rc = accum_alloc(acc, sum_bytes, &W.sum, fn)) != RT_OK || (rc = accum_alloc(acc, n_mats, &table, fn)) != RT_OK)
        return rc; // what was allocated stays with the accumulator's arena, unused, until rt_accum_destroy
    auto queue = [&]() -> int { // `bytes` is a local: nothing of this may be in flight when it dies
        HIP_TRY(hipMemsetAsync(W.sum, 0, sum_bytes, s->stream)); // +0.0
        if (n_mats)
            HIP_TRY(hipMemcpyAsync(table, bytes.data(), n_mats, hipMemcpyHostToDevice, s->stream));
        return RT_OK;
    };
    if ((rc = rt::queue_and_wait(s->stream, queue)) != RT_OK)
        return rc;
    W.material_group = table;
    acc->G = W;
    acc->groups = true;
    return RT_OK;
}

static int groups_check(const rt_accum *acc, const void *buffer, uint32_t flags, const char *fn) {
    if (!acc)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null accumulator");
    if (!acc->groups)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the accumulator has no light groups (rt_accum_attach_light_groups)");
    if (!buffer || (flags & ~(uint32_t)RT_FLAG_DEVICE_FB))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null buffer or flags other than RT_FLAG_DEVICE_FB");
    return RT_OK;
}

extern "C" int rt_accum_read_light_groups(rt_accum *acc, float *group_sums) {
    if (int rc = groups_check(acc, group_sums, 0u, "rt_accum_read_light_groups"); rc != RT_OK)
        return rc;
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    return read_back(s, {{group_sums, acc->G.sum, 12 * (size_t)acc->G.n_groups * acc->G.pixels}});
}

extern "C" int rt_accum_resolve_light_group(rt_accum *acc, uint32_t group, uint32_t flags, float *fb_rgb) {
    if (int rc = groups_check(acc, fb_rgb, flags, "rt_accum_resolve_light_group"); rc != RT_OK)
        return rc;
    if (group >= acc->G.n_groups)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_resolve_light_group: group " + std::to_string(group) + " of " + std::to_string(acc->G.n_groups));
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    rt::CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    float *d_fb;
    io.out(&d_fb, fb_rgb, (size_t)acc->width * acc->height * 12);
    return io.run([&]() -> int {
        HIP_TRY(rt::launch_accum_light_group(acc->R, acc->G, group, d_fb, s->stream));
        return RT_OK;
    });
}

// the G x 3 weights of a mix, as the kernel argument they travel in
static int mix_weights(const rt_accum *acc, const float *weights, const char *fn, rt::LightMixWeights *w) {
    if (!weights)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null weights");
    std::memset(w, 0, sizeof(*w));
    std::memcpy(w->w, weights, 12 * (size_t)acc->G.n_groups);
    return RT_OK;
}

extern "C" int rt_accum_resolve_light_mix(rt_accum *acc, const float *weights, uint32_t flags, float *fb_rgb) {
    rt::LightMixWeights w;
    int rc;
    if ((rc = groups_check(acc, fb_rgb, flags, "rt_accum_resolve_light_mix")) != RT_OK || (rc = mix_weights(acc, weights, "rt_accum_resolve_light_mix", &w)) != RT_OK)
        return rc;
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    rt::CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    float *d_fb;
    io.out(&d_fb, fb_rgb, (size_t)acc->width * acc->height * 12);
    return io.run([&]() -> int {
        HIP_TRY(rt::launch_accum_light_mix(acc->R, acc->G, w, d_fb, s->stream));
        return RT_OK;
    });
}

extern "C" int rt_accum_resolve_light_mix_rgb8(rt_accum *acc, const float *weights, uint32_t flags, uint8_t *rgb8) {
    rt::LightMixWeights w;
    int rc;
    if ((rc = groups_check(acc, rgb8, flags, "rt_accum_resolve_light_mix_rgb8")) != RT_OK || (rc = mix_weights(acc, weights, "rt_accum_resolve_light_mix_rgb8", &w)) != RT_OK)
        return rc;
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    return film_image(acc, flags, rgb8, [&](float *d_fb) { return rt::launch_accum_light_mix(acc->R, acc->G, w, d_fb, s->stream); });
}
