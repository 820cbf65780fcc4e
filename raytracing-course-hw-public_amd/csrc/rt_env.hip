// rt_env.hip — the tables of a float environment (rt_set_environment, include/rt_abi.h), built on the device, and the two probes of its
// distribution (rt_env_pdf, rt_env_sample). The host computes the H band factors and nothing else.
//   k_env_texels   the caller's rgb triples -> float4 texels
//   k_env_weights  w_ij = M_ij * Omega_i in double: M_ij the largest luminance over the bilinear footprint of cell (i, j)
//   k_env_scan     one block per row: the row's prefix sums in double, in the fixed order the header states, normalised to a float CDF;
//                  run once more over the H row totals it gives the marginal
#include <hip/hip_runtime.h>

#include "rt_dev_env.h"
#include "rt_env.h"
#include "rt_kernels.h"

namespace {

#define ENV_SCAN_THREADS 256u

__global__ __launch_bounds__(256) void k_env_texels(const float *rgb, uint32_t n, float4 *texels) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        texels[i] = make_float4(rgb[3ull * i], rgb[3ull * i + 1], rgb[3ull * i + 2], 0.0f);
}

// A lookup with (x0, y0) = (j, i) reads texels (j, i), (j, i+1), (j+1, i), (j+1, i+1), the successors wrapping like mod_inc: their largest
// luminance bounds the radiance anywhere inside the cell, so the cell's weight is positive wherever its radiance is.
__global__ __launch_bounds__(256) void k_env_weights(const float4 *texels, uint32_t width, uint32_t height, float bg_r, float bg_g, float bg_b, const double *omega,
                                                    double *weights) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= width * height)
        return;
    const uint32_t i = idx / width, j = idx - i * width;
    const uint32_t i1 = i + 1u == height ? 0u : i + 1u, j1 = j + 1u == width ? 0u : j + 1u;
    auto lum = [&](uint32_t y, uint32_t x) {
        const float4 t = texels[(size_t)y * width + x];
        return (0.2126f * (bg_r * t.x) + 0.7152f * (bg_g * t.y)) + 0.0722f * (bg_b * t.z);
    };
    const float m = rmax(rmax(rmax(rmax(0.0f, lum(i, j)), lum(i1, j)), lum(i, j1)), lum(i1, j1));
    weights[idx] = (double)m * omega[i];
}

// Prefix sums of n doubles per row in a fixed order: the row is cut into ENV_SCAN_THREADS chunks of C = ceil(n / 256) consecutive elements;
// L_k = the sum of chunk c's elements up to k, left to right from its first; B_c = the sum of the totals of the chunks before c, left to
// right; P_k = B_c + L_k. cdf[k + 1] = (float)(P_k / P_(n-1)), cdf[0] = 0, cdf[n] = 1; a row whose total is 0 gets (k + 1) / n (nothing
// selects it). total[row] = P_(n-1).
__global__ __launch_bounds__(ENV_SCAN_THREADS) void k_env_scan(const double *w, uint32_t n, float *cdf, double *total) {
    __shared__ double s_tot[ENV_SCAN_THREADS];
    __shared__ double s_base[ENV_SCAN_THREADS + 1u];
    const uint32_t row = blockIdx.x, t = threadIdx.x;
    const uint32_t chunk = (n + ENV_SCAN_THREADS - 1u) / ENV_SCAN_THREADS;
    const uint32_t begin = t * chunk < n ? t * chunk : n, end = begin + chunk < n ? begin + chunk : n;
    const double *wr = w + (size_t)row * n;
    float *out = cdf + (size_t)row * (n + 1u);
    double acc = 0.0;
    for (uint32_t k = begin; k < end; ++k)
        acc += wr[k];
    s_tot[t] = acc;
    __syncthreads();
    if (t == 0u) {
        double b = 0.0;
        for (uint32_t c = 0; c < ENV_SCAN_THREADS; ++c) {
            s_base[c] = b;
            b += s_tot[c];
        }
        s_base[ENV_SCAN_THREADS] = b;
        total[row] = b;
        out[0] = 0.0f;
    }
    __syncthreads();
    const double sum = s_base[ENV_SCAN_THREADS], base = s_base[t];
    acc = 0.0;
    for (uint32_t k = begin; k < end; ++k) {
        acc += wr[k];
        float v = sum > 0.0 ? (float)((base + acc) / sum) : (float)(k + 1u) / (float)n;
        if (k + 1u == n)
            v = 1.0f;
        out[k + 1u] = v;
    }
}

__global__ __launch_bounds__(256) void k_env_pdf(const DevEnv E, const float *dirs, uint32_t n, float *pdf_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        pdf_out[i] = env_pdf(E, ld3(dirs + 3ull * i));
}

__global__ __launch_bounds__(256) void k_env_sample(const DevEnv E, const float *xi4, uint32_t n, float *dirs_out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const float4 x = reinterpret_cast<const float4 *>(xi4)[i];
    const V3 d = env_sample_xi(E, x.x, x.y, x.z, x.w);
    dirs_out[3ull * i] = d.x;
    dirs_out[3ull * i + 1] = d.y;
    dirs_out[3ull * i + 2] = d.z;
}

} // namespace

namespace rt {

hipError_t launch_env_build(const DevEnv &E, const EnvBuild &B, const float *bg, bool dist, hipStream_t stream) {
    const uint32_t n = E.width * E.height; // <= 2^25
    float4 *texels = reinterpret_cast<float4 *>(const_cast<float *>(E.texels));
    hipError_t e = RT_LAUNCH_CHECKED(k_env_texels, dim3((n + 255u) / 256u), dim3(256), 0, stream, B.rgb, n, texels);
    if (e != hipSuccess || !dist)
        return e;
    if ((e = RT_LAUNCH_CHECKED(k_env_weights, dim3((n + 255u) / 256u), dim3(256), 0, stream, texels, E.width, E.height, bg[0], bg[1], bg[2], B.omega, B.weights)) != hipSuccess)
        return e;
    if ((e = RT_LAUNCH_CHECKED(k_env_scan, dim3(E.height), dim3(ENV_SCAN_THREADS), 0, stream, B.weights, E.width, const_cast<float *>(E.rows), B.row_total)) != hipSuccess)
        return e;
    return RT_LAUNCH_CHECKED(k_env_scan, dim3(1), dim3(ENV_SCAN_THREADS), 0, stream, B.row_total, E.height, const_cast<float *>(E.marg), B.total);
}

hipError_t launch_env_pdf(const DevEnv &E, const float *dirs, uint32_t n, float *pdf, hipStream_t stream) {
    if (n == 0)
        return hipSuccess;
    return RT_LAUNCH_CHECKED(k_env_pdf, dim3((n + 255u) / 256u), dim3(256), 0, stream, E, dirs, n, pdf);
}

hipError_t launch_env_sample(const DevEnv &E, const float *xi4, uint32_t n, float *dirs, hipStream_t stream) {
    if (n == 0)
        return hipSuccess;
    return RT_LAUNCH_CHECKED(k_env_sample, dim3((n + 255u) / 256u), dim3(256), 0, stream, E, xi4, n, dirs);
}

} // namespace rt
