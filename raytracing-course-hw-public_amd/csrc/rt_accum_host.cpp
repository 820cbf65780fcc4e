// rt_accum_host.cpp — the host side of the accumulators (rt_abi.h rt_accum_*; their kernels are rt_accum.hip): create and destroy, the
// rounds of rt_accum_render*, the image and the state. The optional layers' own entry points are rt_accum_layers.cpp.
//
// An accumulator owns its per-pixel state (S, E, n, err, the round's target and list, about 64 B per pixel) and one camera record; it
// borrows the scene's stream, its wavefront workspace and its staging block (rt_call_io.h). Every call ends with the stream synchronised, so an
// rt_render on the same scene in between only ever sees an idle workspace, and never touches the accumulator's buffers.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rt_accum_impl.h"

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
    if (s->shutter_accums)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_create: the scene has an accumulator with a shutter, which moves its geometry: destroy it first");
    HIP_TRY(hipSetDevice(s->device));
    auto a = std::make_unique<rt_accum>();
    a->scene = s;
    a->width = width;
    a->height = height;
    if (sensor) {
        if (int rc = rt::check_sensor(*sensor, width, height, "rt_accum_create_sensor"); rc != RT_OK)
            return rc;
        a->sensor_desc = *sensor;
    } else { // the pinhole record of {camera, seed}, as rt::make_sensor(camera, seed) states it
        a->sensor_desc.camera = camera ? *camera : s->cam;
        a->sensor_desc.kind = RT_SENSOR_PINHOLE;
        a->sensor_desc.seed = seed;
    }
    a->sensor = rt::make_sensor(a->sensor_desc, width, height);
    const size_t n = (size_t)width * height;
    auto alloc = [&]<class T>(size_t bytes, T **ptr) -> int { return rt::accum_alloc(a.get(), bytes, ptr, "rt_accum_create"); };
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
        WfFeat F{};
        if ((rc = alloc(12 * n, &F.albedo_sum)) != RT_OK || (rc = alloc(12 * n, &F.normal_sum)) != RT_OK || (rc = alloc(4 * n, &F.depth_sum)) != RT_OK ||
            (rc = alloc(4 * n, &F.hits)) != RT_OK)
            return rc;
        HIP_TRY(hipMemsetAsync(F.albedo_sum, 0, 12 * n, s->stream)); // +0.0
        HIP_TRY(hipMemsetAsync(F.normal_sum, 0, 12 * n, s->stream));
        HIP_TRY(hipMemsetAsync(F.depth_sum, 0, 4 * n, s->stream));
        HIP_TRY(hipMemsetAsync(F.hits, 0, 4 * n, s->stream));
        a->features = F;
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
    WfFeat *const F = rt::layer_ptr(a->features); // the layers it keeps (null: not this one): their per-path records are bound per fill
    WfIds *const I = rt::layer_ptr(a->ids);
    WfGroups *const G = rt::layer_ptr(a->groups);
    WfFlow *const Fl = rt::layer_ptr(a->flow);
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
            if (int rc = s->bind_layer_records(F, I, G, Fl); rc != RT_OK)
                return rc;
            s->wf_bind(W);
            W.fb = nullptr;
            W.accum = nullptr; // wf_resolve does not run on an accumulator pass
            for (uint32_t e0 = 0; e0 < tot[0]; e0 += per_pass) {
                WfAccum A{a->R.sum, a->R.even_sum, a->R.count, a->R.list_pix, a->R.list_base, a->R.list_off, e0, std::min(per_pass, tot[0] - e0)};
                W.n_paths = (uint32_t)std::min<uint64_t>((uint64_t)A.n_entries * C, tot[1]); // an upper bound: the first stage reads the exact count
                W.first_pixel = 0, W.pass_pixels = A.n_entries;
                W.first_sample = 0, W.pass_samples = C, W.samples = C;
                a->has_samples = true;
                const rt::WfPassKind kind = rt::WfPassKind::list(A, rt::WfLayers{F, I, G, Fl}, a->sensor);
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

    // the uniform step: `samples` more for every pixel
    auto uniform = [&](uint32_t samples) -> int {
        HIP_TRY(rt::launch_accum_uniform(a->R, samples, s->stream));
        bool any = false;
        return fill(samples, &any);
    };
    // ... of an accumulator with a shutter (rt_abi.h rt_accum_attach_shutter): the call's sample range in maximal runs of one slice, each
    // through the uniform step on the scene and the view of its slice; then key 0 again, whatever happened
    auto shutter_runs = [&]() -> int {
        rt::Shutter &H = *a->shutter;
        H.change_ms = 0, H.changes = 0;
        int rc = RT_OK;
        for (uint64_t n = H.n_samples, end = n + p->samples; n < end && rc == RT_OK;) {
            const uint32_t len = (uint32_t)(H.slices == 1 ? end - n : std::min<uint64_t>(end - n, H.block - n % H.block));
            if ((rc = rt::shutter_install(a, (int)rt::shutter_slice(H, n))) == RT_OK && (rc = uniform(len)) == RT_OK)
                H.n_samples = n += len;
        }
        const int back = rt::shutter_install(a, -1);
        return rc != RT_OK ? rc : back;
    };

    auto rounds_of_call = [&]() -> int {
        if (!ad) {
            if (int rc = a->shutter ? shutter_runs() : uniform(p->samples); rc != RT_OK)
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
    if (acc->shutter)
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_accum_render_adaptive: the accumulator has a shutter; per-pixel sample counts would put one pass at several times");
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

template <class Out> static int resolve(rt_accum *acc, uint32_t flags, Out *out, const char *fn) {
    if (!acc || !out || rt::other_flags(flags))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null argument or flags other than RT_FLAG_DEVICE_FB");
    return rt::accum_image(acc, flags, out, [&](float *d_fb) { return rt::launch_accum_image(acc->R, d_fb, acc->scene->stream); });
}
extern "C" int rt_accum_resolve(rt_accum *acc, uint32_t flags, float *fb_rgb) { return resolve(acc, flags, fb_rgb, "rt_accum_resolve"); }
extern "C" int rt_accum_resolve_rgb8(rt_accum *acc, uint32_t flags, uint8_t *rgb8) { return resolve(acc, flags, rgb8, "rt_accum_resolve_rgb8"); }

extern "C" int rt_accum_read(rt_accum *acc, float *sum_rgb, float *even_sum_rgb, uint32_t *samples, float *error) {
    if (int rc = rt::accum_entry(acc, "rt_accum_read", rt::AccumNeed::NONE); rc != RT_OK)
        return rc;
    const size_t n = (size_t)acc->width * acc->height;
    return rt::read_back(acc, {{sum_rgb, acc->R.sum, 12 * n}, {even_sum_rgb, acc->R.even_sum, 12 * n}, {samples, acc->R.count, 4 * n}, {error, acc->R.err, 4 * n}});
}
