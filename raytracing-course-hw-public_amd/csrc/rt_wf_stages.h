// rt_wf_stages.h — the two ends of a wavefront pass on the device (part of rt_wavefront.hip's translation unit): the first stage, written
// once over the four sources a pass's paths can come from (rt_kernels.h WfPassKind), wf_fold, the last stages that add a pass's finished
// samples where its kind keeps them, and the two writers that deliver first rays as rt_ray records (rt_sensor_rays, rt_bake_rays). What runs
// between the ends is rt_wf_extend.hip's (or rt_wide.hip's), rt_wf_shade.hip's and, with the launchers of a pass, rt_wavefront.hip's (sort, advance).
#pragma once
#include "rt_dev_bake.h"
#include "rt_dev_queue.h"
#include "rt_dev_sensor.h"
#include "rt_dev_shade.h"
#include "rt_wf_records.h"

namespace {

DEV uint32_t wf_global_pixel(const WfLaunch &L, uint32_t local_pixel) {
    const uint32_t local_block = local_pixel / L.shard_block;
    const uint32_t within = local_pixel - local_block * L.shard_block;
    return (local_block * L.shard_count + L.shard_index) * L.shard_block + within;
}

// ------------------------------------------------------------------------------------------------ first stage
// The first record of path i, in queue slot i: the ray (o, d) with `rng` as gen_ray left it (behind its two jitter draws), full budget, no
// pending frames. The one definition of a path's first record, whatever the source of the ray.
// ENVD: the scene's mix_dist has the environment as a component (ENV_FLOAT_DIST), which next_shade_class must know.
template <bool ENVD> DEV void wf_store_first(const DevScene &S, const WfLaunch &L, uint32_t i, V3 o, V3 d, const Rng<RT_RNG_DEVICE> &rng) {
    wf_store_path(L.paths_in + i, wf_pack(o, d, i, next_shade_class<ENVD>(rng, S.lights.n_tris != 0), L.ray_depth, 0u, rng.g));
}

// A source of first rays: an aggregate {pass, the source's kernel argument `Arg`} made once per lane (what does not depend on the path is
// read there), `count()` is the number of paths the first bounce's queue holds, and `ray(i, o, d, rng)` makes path i's ray and stream, or
// returns false where the source has no path i.

// Cameras: path i is sample first_sample + ds of local pixel first_pixel + lp; its ray is sensor_ray (rt_dev_sensor.h) of the camera that
// holds the pixel in the virtual (view-major) image, L.sensors[vpix / view_pixels]. A view of rt_render* is a pinhole record, whose branch
// of sensor_ray is gen_ray (raytracer.h:527-538) itself. The list source draws from the same function, so sample s of pixel p is the same
// ray whichever of them draws it.
struct WfFromCameras {
    struct Arg {};
    const WfLaunch &L;
    Arg none;
    DEV uint32_t count() const { return L.n_paths; }
    DEV bool ray(uint32_t i, V3 &o, V3 &d, Rng<RT_RNG_DEVICE> &rng) const {
        const uint32_t lp = i / L.pass_samples;
        const uint32_t ds = i - lp * L.pass_samples;
        const uint32_t vpix = wf_global_pixel(L, L.first_pixel + lp); // pixel of the virtual (view-major) image
        const uint32_t v = vpix / L.view_pixels;
        sensor_ray_of(L.sensors, v, L.width, L.height, vpix - v * L.view_pixels, L.first_sample + ds,
                      [&](V3 so, V3 sd, const Rng<RT_RNG_DEVICE> &sr) { o = so, d = sd, rng = sr; });
        return true;
    }
};

// An accumulator round's list (WfAccum): path i takes the entry whose prefix range holds off[first] + i (binary search; a pixel's paths stay
// consecutive, so the 64 queue positions of a packet are still the samples of one or a few pixels). The pass's L.n_paths is an upper bound:
// there is no path in [exact count, L.n_paths).
struct WfFromList {
    using Arg = WfAccum;
    const WfLaunch &L;
    const WfAccum &A;
    const uint32_t *off = A.list_off + A.first_entry;
    uint32_t base = off[0], n_exact = off[A.n_entries] - base;
    DEV uint32_t count() const { return n_exact; }
    DEV bool ray(uint32_t i, V3 &o, V3 &d, Rng<RT_RNG_DEVICE> &rng) const {
        if (i >= n_exact)
            return false;
        const uint32_t g = base + i;
        uint32_t lo = 0, hi = A.n_entries - 1; // the last e with off[e] <= g (entries have k >= 1: off is strictly increasing)
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1u) >> 1;
            if (off[mid] <= g)
                lo = mid;
            else
                hi = mid - 1u;
        }
        const uint32_t e = A.first_entry + lo;
        sensor_ray_of(L.sensors, 0u, L.width, L.height, A.list_pix[e], A.list_base[e] + (g - off[lo]), // an accumulator has one camera
                      [&](V3 so, V3 sd, const Rng<RT_RNG_DEVICE> &sr) { o = so, d = sd, rng = sr; });
        return true;
    }
};

// The stream of a path whose ray is not a camera's: seeded from (seed, stream, sample), then gen_ray's two jitter draws, made and discarded
// (raytracer.h:527-538: the stream then stands where a camera ray's stands)
DEV void wf_seed_behind_jitter(Rng<RT_RNG_DEVICE> &rng, uint64_t seed, uint32_t stream, uint32_t sample) {
    rt_xoshiro_seed(&rng.g, seed, stream, sample);
    (void)uniform_real(rng, 0.0f, 1.0f);
    (void)uniform_real(rng, 0.0f, 1.0f);
}

// A caller's rays (WfRays, rt_render_rays): path i is sample index first_sample + ds of output first_pixel + lp, like a camera's, and that is
// sample `first_sample + ds % K` of ray `output * G + ds / K` of the caller's buffer. The lane reads its 32-byte record as two 16-byte pieces
// (with K = 1 the lanes of a wave read consecutive records), seeds the stream the record names and stores the ray as given: no normalisation.
struct WfFromRays {
    using Arg = WfRays;
    const WfLaunch &L;
    const WfRays &R;
    DEV uint32_t count() const { return L.n_paths; }
    DEV bool ray(uint32_t i, V3 &o, V3 &d, Rng<RT_RNG_DEVICE> &rng) const {
        const uint4 *recs = reinterpret_cast<const uint4 *>(R.rays);
        const uint32_t lp = i / L.pass_samples;
        const uint32_t ds = L.first_sample + (i - lp * L.pass_samples); // < G * K
        const uint32_t sub = ds / R.samples;                            // < G
        const size_t ray = (size_t)(L.first_pixel + lp) * R.group + sub;
        const uint4 p0 = recs[2 * ray], p1 = recs[2 * ray + 1];
        wf_seed_behind_jitter(rng, R.seed, p1.z, p1.w + (ds - sub * R.samples)); // the sample index wraps mod 2^32
        o = mk(__uint_as_float(p0.x), __uint_as_float(p0.y), __uint_as_float(p0.z));
        d = mk(__uint_as_float(p0.w), __uint_as_float(p1.x), __uint_as_float(p1.y));
        return true;
    }
};

// Bake points (WfBake, rt_bake): path i is sample S = bake.first_sample + first_sample + ds of point first_pixel + lp. The lane reads the
// point's 32-byte record as two 16-byte pieces, seeds the path's stream from (seed, point.stream, S) and asks bake_ray (rt_dev_bake.h) for
// the ray: the rt_ray record rt_bake_rays writes for (point, S) is this ray.
struct WfFromBake {
    using Arg = WfBake;
    const WfLaunch &L;
    const WfBake &B;
    DEV uint32_t count() const { return L.n_paths; }
    DEV bool ray(uint32_t i, V3 &o, V3 &d, Rng<RT_RNG_DEVICE> &rng) const {
        const uint4 *recs = reinterpret_cast<const uint4 *>(B.points);
        const uint32_t lp = i / L.pass_samples;
        const uint32_t smp = B.first_sample + (L.first_sample + (i - lp * L.pass_samples)); // the sample index wraps mod 2^32
        const size_t pt = (size_t)(L.first_pixel + lp);
        const uint4 p0 = recs[2 * pt], p1 = recs[2 * pt + 1];
        wf_seed_behind_jitter(rng, B.seed, p1.z, smp);
        bake_ray(B.kind, B.offset, B.seed, p0, p1, smp, o, d);
        return true;
    }
};

// The first stage of every pass: the first bounce's queue is the identity (slot i holds path i) over the source's count. A path the source
// does not have gets an empty finished sample (no frames), so that wf_fold, which runs over L.n_paths, reads nothing stale.
template <bool STATS, bool ENVD, class SRC> __global__ __launch_bounds__(256) void wf_first_stage(const DevScene S, const WfLaunch L, const typename SRC::Arg arg) {
    LaneStats<STATS> st;
    const SRC src{L, arg};
    if (blockIdx.x == 0 && threadIdx.x == 0)
        L.counters[WF_CNT_IN] = src.count();
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < L.n_paths; i += gridDim.x * blockDim.x) {
        V3 o, d;
        Rng<RT_RNG_DEVICE> rng;
        if (!src.ray(i, o, d, rng)) {
            L.sample_out[i] = RtF4{0.f, 0.f, 0.f, __uint_as_float(0u)};
            continue;
        }
        wf_store_first<ENVD>(S, L, i, o, d, rng);
        st.cast(); // ray_depth >= 1: trace_ray casts (raytracer.h:600)
    }
    st.flush(L.stats);
}

// ------------------------------------------------------------------------------------------------ first rays as rt_ray records
// One rt_ray record {o, d, stream, first_sample} (rt_abi.h) at out[2 * i]: two 16-byte pieces per lane (consecutive lanes, consecutive
// records). The RNG state is not kept: the rays source reseeds from (stream, first_sample) and repeats the two draws.
DEV void wf_store_ray_record(uint4 *out, uint32_t i, V3 o, V3 d, uint32_t stream, uint32_t sample) {
    out[2ull * i] = make_uint4(__float_as_uint(o.x), __float_as_uint(o.y), __float_as_uint(o.z), __float_as_uint(d.x));
    out[2ull * i + 1] = make_uint4(__float_as_uint(d.y), __float_as_uint(d.z), stream, sample);
}

// rt_bake_rays: record i of the output is sample first_sample + i % samples of point i / samples, with the point's stream
__global__ __launch_bounds__(256) void wf_bake_rays(const WfBake B, uint32_t samples, uint32_t n, uint4 *out) {
    const uint4 *recs = reinterpret_cast<const uint4 *>(B.points);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t pt = i / samples;
        const uint32_t smp = B.first_sample + (i - pt * samples);
        const uint4 p0 = recs[2ull * pt], p1 = recs[2ull * pt + 1];
        V3 o, d;
        bake_ray(B.kind, B.offset, B.seed, p0, p1, smp, o, d);
        wf_store_ray_record(out, i, o, d, p1.z, smp);
    }
}

// rt_sensor_rays: record i of the output is sample first_sample + i % samples of pixel first_pixel + i / samples of the one sensor
// `sensor[0]`, with the pixel as its stream
__global__ __launch_bounds__(256) void wf_sensor_rays(const WfSensor *sensor, uint32_t width, uint32_t height, uint32_t first_pixel, uint32_t first_sample, uint32_t samples,
                                                      uint32_t n, uint4 *out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t lp = i / samples;
        const uint32_t pix = first_pixel + lp, s = first_sample + (i - lp * samples);
        sensor_ray_of(sensor, 0u, width, height, pix, s, [&](V3 o, V3 d, const Rng<RT_RNG_DEVICE> &) { wf_store_ray_record(out, i, o, d, pix, s); });
    }
}

// ------------------------------------------------------------------------------------------------ fold
// The return path of the recursion (raytracer.h:588-590): every finished path's pending frames `emission + inner * scl`, innermost
// first, then sanitize_nans (:607-616). One lane per path of the pass, all lanes busy; frames are stored level by level (WfLaunch::fold), so a
// wave reads 1 KB of consecutive scale records per level, the emission records only of the frames that have one, and nothing it does not need.
__global__ __launch_bounds__(256) void wf_fold(const WfLaunch L) {
    for (uint32_t path = blockIdx.x * blockDim.x + threadIdx.x; path < L.n_paths; path += gridDim.x * blockDim.x) {
        const RtF4 v = L.sample_out[path];
        V3 res = mk(v.x, v.y, v.z);
        uint32_t nb = __float_as_uint(v.w);
        while (nb > 0) {
            --nb;
            V3 emission, scl;
            wf_load_fold(L, nb, path, emission, scl); // frame level nb: adjacent lanes, adjacent records; the emission record only where flagged
            const V3 clr = res * scl;
            res = emission + clr;
        }
        if (isnan_f(res.x))
            res.x = 0;
        if (isnan_f(res.y))
            res.y = 0;
        if (isnan_f(res.z))
            res.z = 0;
        L.sample_out[path] = RtF4{res.x, res.y, res.z, 0.f};
    }
}

// The same fold once more for a pass of an accumulator with light groups (WfGroups; the rule: rt_abi.h rt_accum_attach_light_groups), before
// wf_fold, which overwrites sample_out: V_g of every path, for all groups at once. One lane per path reads the terminal value and then each
// frame level once, through wf_load_fold like wf_fold, and the byte tag of that level; group g's running value takes the terminal value or a
// frame's emission where the tag equals g and (+0, +0, +0) elsewhere, in the float operations of wf_fold. A tag is only ever compared: a
// stale one (WfGroups) stands beside a value that is exactly +0. The eight running values are named by constant indices of unrolled loops
// (registers, no private array in memory); the loops run to RT_LIGHT_GROUP_MAX whatever G is, and only the G records are stored, group-major.
__global__ __launch_bounds__(256) void wf_fold_groups(const WfLaunch L, const WfGroups Gr) {
    for (uint32_t path = blockIdx.x * blockDim.x + threadIdx.x; path < L.n_paths; path += gridDim.x * blockDim.x) {
        const RtF4 v = L.sample_out[path];
        const V3 term = mk(v.x, v.y, v.z);
        uint32_t nb = __float_as_uint(v.w);
        const uint32_t t_tag = Gr.tag[wf_fold_index(L.n_paths, nb, path)];
        V3 res[RT_LIGHT_GROUP_MAX];
#pragma unroll
        for (uint32_t g = 0; g < RT_LIGHT_GROUP_MAX; ++g)
            res[g] = t_tag == g ? term : mk(0.f, 0.f, 0.f);
        while (nb > 0) {
            --nb;
            V3 emission, scl;
            wf_load_fold(L, nb, path, emission, scl);
            const uint32_t tag = Gr.tag[wf_fold_index(L.n_paths, nb, path)];
#pragma unroll
            for (uint32_t g = 0; g < RT_LIGHT_GROUP_MAX; ++g) {
                const V3 clr = res[g] * scl;
                res[g] = (tag == g ? emission : mk(0.f, 0.f, 0.f)) + clr;
            }
        }
#pragma unroll
        for (uint32_t g = 0; g < RT_LIGHT_GROUP_MAX; ++g) {
            if (g < Gr.n_groups) { // wave-uniform
                V3 r = res[g];
                if (isnan_f(r.x))
                    r.x = 0;
                if (isnan_f(r.y))
                    r.y = 0;
                if (isnan_f(r.z))
                    r.z = 0;
                Gr.rec[wf_fold_index(L.n_paths, g, path)] = RtF4{r.x, r.y, r.z, 0.f};
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ resolve
// render_pixel's `res += sanitize_nans(...)` loop (raytracer.h:621-625) for the samples of this pass, in sample order,
// continuing the running sum of earlier passes; the final pass divides by the sample count (:626).
__global__ __launch_bounds__(256) void wf_resolve(const WfLaunch L, int first_pass, int last_pass) {
    for (uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x; lp < L.pass_pixels; lp += gridDim.x * blockDim.x) {
        V3 acc = mk(0, 0, 0);
        if (!first_pass) {
            const RtF4 a = L.accum[lp];
            acc = mk(a.x, a.y, a.z);
        }
        const RtF4 *src = L.sample_out + (size_t)lp * L.pass_samples;
        for (uint32_t ds = 0; ds < L.pass_samples; ++ds) {
            const RtF4 v = src[ds];
            acc = acc + mk(v.x, v.y, v.z);
        }
        if (last_pass) {
            const V3 out = acc / (float)L.samples;
            float *dst = L.fb + 3ull * wf_global_pixel(L, L.first_pixel + lp);
            dst[0] = out.x;
            dst[1] = out.y;
            dst[2] = out.z;
        } else {
            L.accum[lp] = RtF4{acc.x, acc.y, acc.z, 0.f};
        }
    }
}

// The fold of a pass of rt_bake (WfBake), in wf_resolve's place: one lane per output (point, k) with k < 1 (IRRADIANCE) or k < 9 (SH9) owns its
// three sums and adds the pass's samples in sample order; the nine lanes of an SH point read the same sample records. The sums of earlier
// sample passes are in `out` itself; the last pass divides by the sample count and scales. SH9 weighs sample s by Y_k of its own direction,
// which bake_ray makes again from (seed, stream, S): no direction buffer is kept between the stages.
__global__ __launch_bounds__(256) void wf_resolve_bake(const WfLaunch L, const WfBake B, int first_pass, int last_pass) {
    const bool sh = B.kind == RT_BAKE_SH9;
    const uint32_t nk = sh ? 9u : 1u;
    const uint64_t n = (uint64_t)L.pass_pixels * nk;
    const uint4 *recs = reinterpret_cast<const uint4 *>(B.points);
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t lp = (uint32_t)(t / nk), k = (uint32_t)(t - (uint64_t)lp * nk);
        const size_t pt = (size_t)(L.first_pixel + lp);
        float *dst = B.out + (pt * nk + k) * 3u;
        V3 acc = first_pass ? mk(0, 0, 0) : ld3(dst);
        const RtF4 *src = L.sample_out + (size_t)lp * L.pass_samples;
        if (sh) {
            const uint4 p0 = recs[2 * pt], p1 = recs[2 * pt + 1];
            for (uint32_t ds = 0; ds < L.pass_samples; ++ds) {
                const RtF4 v = src[ds];
                V3 o, d;
                bake_ray(B.kind, B.offset, B.seed, p0, p1, B.first_sample + (L.first_sample + ds), o, d);
                const float y = bake_sh9(k, d);
                acc = acc + mk(v.x * y, v.y * y, v.z * y);
            }
        } else {
            for (uint32_t ds = 0; ds < L.pass_samples; ++ds) {
                const RtF4 v = src[ds];
                acc = acc + mk(v.x, v.y, v.z);
            }
        }
        if (last_pass)
            acc = (acc / (float)L.samples) * (sh ? 4.0f * PI_F : PI_F);
        dst[0] = acc.x;
        dst[1] = acc.y;
        dst[2] = acc.z;
    }
}

// The same loop for an accumulator pass: one lane per entry adds its k consecutive samples onto S_p, and the even-index ones onto E_p,
// in sample order, then n_p += k. A pixel has at most one entry per round, so the lane owns the pixel's sums; no division here.
__global__ __launch_bounds__(256) void wf_resolve_list(const WfLaunch L, const WfAccum A) {
    const uint32_t *off = A.list_off + A.first_entry;
    for (uint32_t le = blockIdx.x * blockDim.x + threadIdx.x; le < A.n_entries; le += gridDim.x * blockDim.x) {
        const uint32_t e = A.first_entry + le, p = A.list_pix[e], s0 = A.list_base[e];
        const uint32_t k = off[le + 1] - off[le];
        V3 acc = ld3(A.sum + 3ull * p), ev = ld3(A.even_sum + 3ull * p);
        const RtF4 *src = L.sample_out + (off[le] - off[0]);
        for (uint32_t j = 0; j < k; ++j) {
            const RtF4 v = src[j];
            acc = acc + mk(v.x, v.y, v.z);
            if (((s0 + j) & 1u) == 0u)
                ev = ev + mk(v.x, v.y, v.z);
        }
        A.sum[3ull * p] = acc.x, A.sum[3ull * p + 1] = acc.y, A.sum[3ull * p + 2] = acc.z;
        A.even_sum[3ull * p] = ev.x, A.even_sum[3ull * p + 1] = ev.y, A.even_sum[3ull * p + 2] = ev.z;
        A.count[p] = s0 + k;
    }
}

// The feature sums of the same entries (WfFeat): the lane that owns the pixel adds its k records in sample order. Runs before
// wf_resolve_list of the pass (it reads the entry's base count from the list, never n_p).
__global__ __launch_bounds__(256) void wf_resolve_features(const WfAccum A, const WfFeat F) {
    const uint32_t *off = A.list_off + A.first_entry;
    for (uint32_t le = blockIdx.x * blockDim.x + threadIdx.x; le < A.n_entries; le += gridDim.x * blockDim.x) {
        const uint32_t p = A.list_pix[A.first_entry + le];
        const uint32_t k = off[le + 1] - off[le];
        V3 al = ld3(F.albedo_sum + 3ull * p), nr = ld3(F.normal_sum + 3ull * p);
        float z = F.depth_sum[p];
        uint32_t hits = F.hits[p];
        const RtF4 *src = F.rec + 2ull * (off[le] - off[0]);
        for (uint32_t j = 0; j < k; ++j) {
            const RtF4 r0 = src[2u * j], r1 = src[2u * j + 1u];
            al = al + mk(r0.x, r0.y, r0.z);
            nr = nr + mk(r1.x, r1.y, r1.z);
            z = z + r0.w;
            hits += __float_as_uint(r1.w);
        }
        F.albedo_sum[3ull * p] = al.x, F.albedo_sum[3ull * p + 1] = al.y, F.albedo_sum[3ull * p + 2] = al.z;
        F.normal_sum[3ull * p] = nr.x, F.normal_sum[3ull * p + 1] = nr.y, F.normal_sum[3ull * p + 2] = nr.z;
        F.depth_sum[p] = z;
        F.hits[p] = hits;
    }
}

// The group sums of the same entries (WfGroups): the lane that owns the pixel adds its k records of every group onto GS_g,p in sample order,
// one group after the other (G is a run-time value: the sums stay in memory, [g][p][3], and one V3 is live at a time). Runs before
// wf_resolve_list of the pass and reads neither n_p nor the base count. `n_paths` is the pass's WfLaunch::n_paths, the stride of the records.
__global__ __launch_bounds__(256) void wf_resolve_groups(const WfAccum A, const WfGroups Gr, uint32_t n_paths) {
    const uint32_t *off = A.list_off + A.first_entry;
    for (uint32_t le = blockIdx.x * blockDim.x + threadIdx.x; le < A.n_entries; le += gridDim.x * blockDim.x) {
        const uint32_t p = A.list_pix[A.first_entry + le];
        const uint32_t k = off[le + 1] - off[le];
        for (uint32_t g = 0; g < Gr.n_groups; ++g) {
            float *dst = Gr.sum + 3ull * ((size_t)g * Gr.pixels + p);
            V3 acc = ld3(dst);
            const RtF4 *src = Gr.rec + wf_fold_index(n_paths, g, off[le] - off[0]);
            for (uint32_t j = 0; j < k; ++j) {
                const RtF4 v = src[j];
                acc = acc + mk(v.x, v.y, v.z);
            }
            dst[0] = acc.x, dst[1] = acc.y, dst[2] = acc.z;
        }
    }
}

// The id tables of the same entries (WfIds; the rule: rt_abi.h rt_accum_attach_ids): the lane that owns the pixel takes its k ids in sample
// order. Runs before wf_resolve_list of the pass, like wf_resolve_features, and reads neither n_p nor the base count: the table itself is the
// state. K is a run-time value, so the slots are walked in memory (slot-major: a wave's lanes stay coalesced), never in a private array. A
// sample equal to the one before it, the common case, goes to the slot that one went to without a walk.
__global__ __launch_bounds__(256) void wf_resolve_ids(const WfAccum A, const WfIds I) {
    const uint32_t *off = A.list_off + A.first_entry;
    for (uint32_t le = blockIdx.x * blockDim.x + threadIdx.x; le < A.n_entries; le += gridDim.x * blockDim.x) {
        const uint32_t p = A.list_pix[A.first_entry + le];
        const uint32_t k = off[le + 1] - off[le];
        const uint32_t *src = I.rec + (off[le] - off[0]);
        uint32_t *sid = I.slot_id + p, *cnt = I.slot_count + p;
        uint32_t other = I.other[p];
        uint32_t last_id = 0u, last_j = I.k; // last_j == K: no slot known for last_id
        for (uint32_t s = 0; s < k; ++s) {
            const uint32_t id = src[s];
            if (last_j < I.k && id == last_id) {
                cnt[(size_t)last_j * I.pixels] += 1u;
                continue;
            }
            uint32_t j = 0;
            for (; j < I.k; ++j) {
                const size_t w = (size_t)j * I.pixels;
                const uint32_t c = cnt[w];
                if (c == 0u) { // the lowest empty slot: every slot below it holds another id
                    sid[w] = id;
                    cnt[w] = 1u;
                    break;
                }
                if (sid[w] == id) {
                    cnt[w] = c + 1u;
                    break;
                }
            }
            if (j == I.k)
                other += 1u;
            last_id = id, last_j = j;
        }
        I.other[p] = other;
    }
}

// The motion vectors of the same entries (WfFlow; the rule: rt_abi.h rt_accum_attach_flow): the lane that owns the pixel takes its k records
// in sample order: a valid one is added onto FS_p and counted in m_p, and replaces (NT_p, NF_p) where it is the pixel's first valid sample or
// strictly nearer. Runs before wf_resolve_list of the pass and reads neither n_p nor the base count: the four values are the state.
__global__ __launch_bounds__(256) void wf_resolve_flow(const WfAccum A, const WfFlow Fl) {
    const uint32_t *off = A.list_off + A.first_entry;
    for (uint32_t le = blockIdx.x * blockDim.x + threadIdx.x; le < A.n_entries; le += gridDim.x * blockDim.x) {
        const uint32_t p = A.list_pix[A.first_entry + le];
        const uint32_t k = off[le + 1] - off[le];
        float sx = Fl.flow_sum[2ull * p], sy = Fl.flow_sum[2ull * p + 1];
        float nx = Fl.near_flow[2ull * p], ny = Fl.near_flow[2ull * p + 1], nt = Fl.near_t[p];
        uint32_t m = Fl.valid[p];
        const RtF4 *src = Fl.rec + (off[le] - off[0]);
        for (uint32_t j = 0; j < k; ++j) { // selects, no branch: the loads of later records need not wait for this one's test
            const RtF4 r = src[j];
            const bool valid = __float_as_uint(r.w) != 0u;
            const bool nearer = valid && (m == 0u || r.z < nt);
            sx = valid ? sx + r.x : sx; // (an invalid sample adds nothing, not +0: the sign of a zero sum stays)
            sy = valid ? sy + r.y : sy;
            nx = nearer ? r.x : nx;
            ny = nearer ? r.y : ny;
            nt = nearer ? r.z : nt;
            m += valid ? 1u : 0u;
        }
        Fl.flow_sum[2ull * p] = sx, Fl.flow_sum[2ull * p + 1] = sy;
        Fl.near_flow[2ull * p] = nx, Fl.near_flow[2ull * p + 1] = ny;
        Fl.near_t[p] = nt;
        Fl.valid[p] = m;
    }
}
} // namespace
