// rt_accum.hip — the per-round kernels of the sample accumulators (include/rt_abi.h rt_accum_*).
//
// A round of an accumulator is: judge (which pixels get how many new samples), plan (the list of entries (p, k_p) in pixel order and the
// exclusive prefix of k_p), then the wavefront pipeline's passes over that list (rt_wf_stages.h: the first stage over WfFromList, the unchanged
// extend / shade / fold kernels, wf_resolve_list). Everything here is O(pixels) with one lane per pixel and no float atomics: the list
// comes out of a deterministic scan, so the same state always plans the same list.
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "rt_dev_math.h"
#include "rt_kernels.h"

namespace {

// err_p of the half-buffer estimate (rt_abi.h, "The adaptive rule"), exactly as the header states it
DEV float accum_err(const rt::AccumRound &R, uint32_t p) {
    const uint32_t n = R.count[p];
    if (n < 2u)
        return INFINITY;
    const uint32_t h = (n + 1u) / 2u;
    const V3 I = ld3(R.sum + 3ull * p) / (float)n, A = ld3(R.even_sum + 3ull * p) / (float)h;
    return (fabsf(I.x - A.x) + fabsf(I.y - A.y) + fabsf(I.z - A.z)) / (1e-4f + sqrtf(I.x + I.y + I.z));
}

__global__ __launch_bounds__(256) void accum_err_kernel(const rt::AccumRound R) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x)
        R.err[p] = accum_err(R, p);
}

// target_p of one round. Round 0: min_samples for the pixels below it. Later rounds: n_p + min(step, max - n_p) for an ACTIVE pixel
// (n_p < max and (n_p < min or some err_q of the clipped 3x3 window is not <= threshold)), n_p for the others.
__global__ __launch_bounds__(256) void accum_target_kernel(const rt::AccumRound R, int round0, float threshold, uint32_t min_samples, uint32_t max_samples,
                                                           uint32_t step) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        const uint32_t n = R.count[p];
        uint32_t t = n;
        if (round0) {
            if (n < min_samples)
                t = min_samples;
        } else if (n < max_samples) {
            bool active = n < min_samples;
            const uint32_t x = p % R.width, y = p / R.width;
            const uint32_t x0 = x > 0u ? x - 1u : 0u, x1 = x + 1u < R.width ? x + 1u : x;
            const uint32_t y0 = y > 0u ? y - 1u : 0u, y1 = y + 1u < R.height ? y + 1u : y;
            for (uint32_t yy = y0; yy <= y1 && !active; ++yy)
                for (uint32_t xx = x0; xx <= x1; ++xx)
                    if (!(R.err[yy * R.width + xx] <= threshold)) { // NaN and +inf are not converged
                        active = true;
                        break;
                    }
            if (active)
                t = n + (step < max_samples - n ? step : max_samples - n);
        }
        R.target[p] = t;
    }
}

__global__ __launch_bounds__(256) void accum_uniform_kernel(const rt::AccumRound R, uint32_t samples) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        const uint32_t n = R.count[p];
        R.target[p] = n + samples < n ? 0xFFFFFFFFu : n + samples; // saturating
    }
}

DEV uint32_t accum_k(const rt::AccumRound &R, uint32_t p, uint32_t chunk) {
    const uint32_t d = R.target[p] - R.count[p];
    return d < chunk ? d : chunk;
}

// scan input: (1 << 32 | k) for a pixel with k > 0 new samples, 0 otherwise. The host keeps pixels x chunk below 2^32, so the low word of
// the 64-bit sum never carries into the entry count.
__global__ __launch_bounds__(256) void accum_plan_values(const rt::AccumRound R, uint32_t chunk, unsigned long long *vals) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        const uint32_t k = accum_k(R, p, chunk);
        vals[p] = k ? (1ull << 32) | k : 0ull;
    }
}

__global__ __launch_bounds__(256) void accum_plan_scatter(const rt::AccumRound R, uint32_t chunk) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        const uint32_t k = accum_k(R, p, chunk);
        const unsigned long long v = R.scan[p];
        const uint32_t e = (uint32_t)(v >> 32), off = (uint32_t)v;
        if (k) {
            R.list_pix[e] = p;
            R.list_base[e] = R.count[p];
            R.list_off[e] = off;
        }
        if (p == n_pix - 1u) { // the end of the prefix, and what the host reads back
            const uint32_t entries = e + (k ? 1u : 0u), total = off + k;
            R.list_off[entries] = total;
            R.totals[0] = entries;
            R.totals[1] = total;
        }
    }
}

// the resolve of rt_render's last pass (wf_resolve: acc / (float)samples) for the accumulated sums
__global__ __launch_bounds__(256) void accum_image_kernel(const rt::AccumRound R, float *fb) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        const uint32_t n = R.count[p];
        V3 out = mk(0, 0, 0);
        if (n != 0u)
            out = ld3(R.sum + 3ull * p) / (float)n;
        fb[3ull * p] = out.x;
        fb[3ull * p + 1] = out.y;
        fb[3ull * p + 2] = out.z;
    }
}

// the feature means of rt_accum_resolve_features: AS / n, NS / n (not renormalised), ZS / h; 0 where the divisor is 0
__global__ __launch_bounds__(256) void accum_feature_means_kernel(const rt::AccumRound R, const WfFeat F, float *albedo, float *normal, float *depth) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        const uint32_t n = R.count[p], h = F.hits[p];
        V3 a = mk(0, 0, 0), nr = mk(0, 0, 0);
        if (n != 0u) {
            a = ld3(F.albedo_sum + 3ull * p) / (float)n;
            nr = ld3(F.normal_sum + 3ull * p) / (float)n;
        }
        if (albedo)
            albedo[3ull * p] = a.x, albedo[3ull * p + 1] = a.y, albedo[3ull * p + 2] = a.z;
        if (normal)
            normal[3ull * p] = nr.x, normal[3ull * p + 1] = nr.y, normal[3ull * p + 2] = nr.z;
        if (depth)
            depth[p] = h != 0u ? F.depth_sum[p] / (float)h : 0.0f;
    }
}

// rt_accum_resolve_labels: the id of the fullest slot (ties: the lowest slot) and its share of n_p; RT_ID_MISS and 0 where n_p = 0
__global__ __launch_bounds__(256) void accum_labels_kernel(const rt::AccumRound R, const WfIds I, uint32_t *label, float *coverage) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        const uint32_t n = R.count[p];
        uint32_t best = 0u, best_j = 0u;
        for (uint32_t j = 0; j < I.k; ++j) {
            const uint32_t c = I.slot_count[(size_t)j * n_pix + p];
            if (c > best)
                best = c, best_j = j;
        }
        if (label)
            label[p] = n != 0u ? I.slot_id[(size_t)best_j * n_pix + p] : RT_ID_MISS;
        if (coverage)
            coverage[p] = n != 0u ? (float)best / (float)n : 0.0f;
    }
}

// rt_accum_resolve_matte: the counts of the slots whose id is in `set` (sorted, no duplicates), summed as integers, over n_p
__global__ __launch_bounds__(256) void accum_matte_kernel(const rt::AccumRound R, const WfIds I, const uint32_t *set, uint32_t n_set, float *matte) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        const uint32_t n = R.count[p];
        uint32_t sum = 0u;
        for (uint32_t j = 0; j < I.k; ++j) {
            const uint32_t c = I.slot_count[(size_t)j * n_pix + p];
            if (c == 0u)
                break; // slots fill from 0 up: the rest are empty too
            const uint32_t id = I.slot_id[(size_t)j * n_pix + p];
            uint32_t lo = 0u, hi = n_set; // the first element >= id
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (set[mid] < id)
                    lo = mid + 1u;
                else
                    hi = mid;
            }
            if (lo < n_set && set[lo] == id)
                sum += c;
        }
        matte[p] = n != 0u ? (float)sum / (float)n : 0.0f;
    }
}

// GS_g,p / (float)n_p of one group, 0 where n_p = 0: accum_image_kernel's quotient of a group sum (rt_abi.h rt_accum_attach_light_groups)
DEV V3 accum_group_mean(const WfGroups &G, uint32_t g, uint32_t p, uint32_t n) {
    if (n == 0u)
        return mk(0, 0, 0);
    return ld3(G.sum + 3ull * ((size_t)g * G.pixels + p)) / (float)n;
}

// rt_accum_resolve_light_group
__global__ __launch_bounds__(256) void accum_light_group_kernel(const rt::AccumRound R, const WfGroups G, uint32_t group, float *fb) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        const V3 out = accum_group_mean(G, group, p, R.count[p]);
        fb[3ull * p] = out.x;
        fb[3ull * p + 1] = out.y;
        fb[3ull * p + 2] = out.z;
    }
}

// rt_accum_resolve_light_mix: per channel acc = +0, then acc = acc + mean_g * w[g][c] for g ascending, one multiplication and one addition each
// (-ffp-contract=off). The weights are a kernel argument (scalar registers); the loop over g is over a run-time G with one V3 live.
__global__ __launch_bounds__(256) void accum_light_mix_kernel(const rt::AccumRound R, const WfGroups G, const rt::LightMixWeights W, float *fb) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        const uint32_t n = R.count[p];
        V3 acc = mk(0, 0, 0);
#pragma unroll
        for (uint32_t g = 0; g < RT_LIGHT_GROUP_MAX; ++g) {
            if (g < G.n_groups) {
                const V3 m = accum_group_mean(G, g, p, n);
                acc = acc + mk(m.x * W.w[g][0], m.y * W.w[g][1], m.z * W.w[g][2]);
            }
        }
        fb[3ull * p] = acc.x;
        fb[3ull * p + 1] = acc.y;
        fb[3ull * p + 2] = acc.z;
    }
}

// rt_accum_resolve_flow: the mean or the nearest sample's flow, and the share of the pixel's samples that have one
__global__ __launch_bounds__(256) void accum_flow_kernel(const rt::AccumRound R, const WfFlow F, uint32_t mode, float *flow, float *mask) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        const uint32_t n = R.count[p], m = F.valid[p];
        if (flow) {
            float x = 0.0f, y = 0.0f;
            if (m != 0u && mode == RT_FLOW_NEAREST)
                x = F.near_flow[2ull * p], y = F.near_flow[2ull * p + 1];
            else if (m != 0u)
                x = F.flow_sum[2ull * p] / (float)m, y = F.flow_sum[2ull * p + 1] / (float)m;
            flow[2ull * p] = x;
            flow[2ull * p + 1] = y;
        }
        if (mask)
            mask[p] = n != 0u ? (float)m / (float)n : 0.0f;
    }
}

dim3 accum_grid(const rt::AccumRound &R) {
    const uint64_t n_pix = (uint64_t)R.width * R.height;
    const uint64_t b = (n_pix + 255u) / 256u;
    return dim3((uint32_t)(b < 4096u ? (b > 0 ? b : 1) : 4096u));
}

} // namespace

namespace rt {

size_t accum_scan_temp_bytes(uint32_t pixels) {
    size_t bytes = 0;
    unsigned long long *p = nullptr;
    (void)rocprim::exclusive_scan(nullptr, bytes, p, p, 0ull, (size_t)pixels, rocprim::plus<unsigned long long>(), (hipStream_t) nullptr);
    return bytes;
}

hipError_t launch_accum_judge(const AccumRound &R, int round0, float threshold, uint32_t min_samples, uint32_t max_samples, uint32_t step, hipStream_t stream) {
    hipError_t e;
    if (!round0 && (e = RT_LAUNCH_CHECKED(accum_err_kernel, accum_grid(R), dim3(256), 0, stream, R)) != hipSuccess)
        return e;
    return RT_LAUNCH_CHECKED(accum_target_kernel, accum_grid(R), dim3(256), 0, stream, R, round0, threshold, min_samples, max_samples, step);
}

hipError_t launch_accum_uniform(const AccumRound &R, uint32_t samples, hipStream_t stream) {
    return RT_LAUNCH_CHECKED(accum_uniform_kernel, accum_grid(R), dim3(256), 0, stream, R, samples);
}

hipError_t launch_accum_plan(const AccumRound &R, uint32_t chunk, hipStream_t stream) {
    hipError_t e;
    if ((e = RT_LAUNCH_CHECKED(accum_plan_values, accum_grid(R), dim3(256), 0, stream, R, chunk, R.scan_in)) != hipSuccess)
        return e;
    size_t bytes = R.scan_temp_bytes;
    if ((e = rocprim::exclusive_scan(R.scan_temp, bytes, R.scan_in, R.scan, 0ull, (size_t)R.width * R.height, rocprim::plus<unsigned long long>(), stream)) != hipSuccess)
        return e;
    return RT_LAUNCH_CHECKED(accum_plan_scatter, accum_grid(R), dim3(256), 0, stream, R, chunk);
}

hipError_t launch_accum_image(const AccumRound &R, float *fb, hipStream_t stream) {
    return RT_LAUNCH_CHECKED(accum_image_kernel, accum_grid(R), dim3(256), 0, stream, R, fb);
}

hipError_t launch_accum_feature_means(const AccumRound &R, const WfFeat &F, float *albedo, float *normal, float *depth, hipStream_t stream) {
    return RT_LAUNCH_CHECKED(accum_feature_means_kernel, accum_grid(R), dim3(256), 0, stream, R, F, albedo, normal, depth);
}

hipError_t launch_accum_labels(const AccumRound &R, const WfIds &I, uint32_t *label, float *coverage, hipStream_t stream) {
    return RT_LAUNCH_CHECKED(accum_labels_kernel, accum_grid(R), dim3(256), 0, stream, R, I, label, coverage);
}

hipError_t launch_accum_matte(const AccumRound &R, const WfIds &I, const uint32_t *set, uint32_t n_set, float *matte, hipStream_t stream) {
    return RT_LAUNCH_CHECKED(accum_matte_kernel, accum_grid(R), dim3(256), 0, stream, R, I, set, n_set, matte);
}

hipError_t launch_accum_light_group(const AccumRound &R, const WfGroups &G, uint32_t group, float *fb, hipStream_t stream) {
    return RT_LAUNCH_CHECKED(accum_light_group_kernel, accum_grid(R), dim3(256), 0, stream, R, G, group, fb);
}

hipError_t launch_accum_light_mix(const AccumRound &R, const WfGroups &G, const LightMixWeights &w, float *fb, hipStream_t stream) {
    return RT_LAUNCH_CHECKED(accum_light_mix_kernel, accum_grid(R), dim3(256), 0, stream, R, G, w, fb);
}

hipError_t launch_accum_flow(const AccumRound &R, const WfFlow &F, uint32_t mode, float *flow, float *mask, hipStream_t stream) {
    return RT_LAUNCH_CHECKED(accum_flow_kernel, accum_grid(R), dim3(256), 0, stream, R, F, mode, flow, mask);
}

} // namespace rt
