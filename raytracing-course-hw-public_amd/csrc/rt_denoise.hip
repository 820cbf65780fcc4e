// rt_denoise.hip — rt_accum_denoise: the edge-avoiding a-trous filter over an accumulator's image (the rule, exactly: include/rt_abi.h).
//
// denoise_prepare turns the accumulator's state into what the iterations read: the working signal L0 = C / den, den, and a 32-byte guide
// record per pixel ({N.xyz, Z}, {s, flags}). denoise_iter runs once per iteration with stride 2^i: a tap costs three 16-byte reads (L, and
// the two halves of the guide record). At strides 1 and 2 the 16x16 pixels of a block read a footprint of 20x20 / 24x24 pixels, 25 taps per
// pixel on 1.6 / 2.3 loaded records per pixel: the block stages it in LDS (19 / 27 KB) and taps from there. From stride 4 on the footprints of
// a block's pixels no longer overlap enough and the taps are plain gathers. Both ways run the same tap arithmetic in the same order
// (dn_pixel), so which lane or block computes a pixel changes no result. Everything is IEEE binary32 without contraction (Makefile).
#include "rt_dev_math.h"
#include "rt_kernels.h"

namespace {

constexpr uint32_t DN_VALID = 1u, DN_HIT = 2u;
constexpr int DN_TILE = 16; // a block is 16 x 16 pixels

// den of a valid pixel q (n > 0), and its image C
DEV void dn_signal(const rt::AccumRound &R, const WfFeat &F, uint32_t q, uint32_t n, uint32_t h, bool demod, V3 &C, V3 &den) {
    const float fn = (float)n;
    C = ld3(R.sum + 3ull * q) / fn;
    den = mk(1.0f, 1.0f, 1.0f);
    if (demod) {
        const V3 alb = ld3(F.albedo_sum + 3ull * q) / fn;
        const float m = (float)(n - h) / fn;
        den = mk((alb.x + m) + 1e-3f, (alb.y + m) + 1e-3f, (alb.z + m) + 1e-3f);
    }
}

// d_q of a valid pixel: the half-buffer difference in units of den
DEV float dn_noise(const rt::AccumRound &R, uint32_t q, uint32_t n, V3 C, V3 den) {
    if (n < 2u)
        return INFINITY;
    const V3 A = ld3(R.even_sum + 3ull * q) / (float)((n + 1u) / 2u);
    return (fabsf(C.x - A.x) / den.x + fabsf(C.y - A.y) / den.y) + fabsf(C.z - A.z) / den.z;
}

__global__ __launch_bounds__(256) void denoise_prepare(const rt::AccumRound R, const WfFeat F, const rt::DenoiseBufs D, int demod) {
    const uint32_t n_pix = R.width * R.height;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_pix; p += gridDim.x * blockDim.x) {
        const uint32_t n = R.count[p];
        RtF4 sig{0.f, 0.f, 0.f, 0.f}, dn{0.f, 0.f, 0.f, 0.f}, g0{0.f, 0.f, 0.f, 0.f}, g1{0.f, __uint_as_float(0u), 0.f, 0.f};
        if (n != 0u) {
            const uint32_t h = F.hits[p];
            V3 C, den;
            dn_signal(R, F, p, n, h, demod != 0, C, den);
            const V3 L0 = C / den;
            const V3 N = ld3(F.normal_sum + 3ull * p) / (float)n;
            const float Z = h != 0u ? F.depth_sum[p] / (float)h : 0.0f;
            // s_p: the mean of d_q over the valid pixels of the clipped 3x3 window, row-major
            const uint32_t x = p % R.width, y = p / R.width;
            const uint32_t x0 = x > 0u ? x - 1u : 0u, x1 = x + 1u < R.width ? x + 1u : x;
            const uint32_t y0 = y > 0u ? y - 1u : 0u, y1 = y + 1u < R.height ? y + 1u : y;
            float sum = 0.0f;
            uint32_t cnt = 0u;
            for (uint32_t yy = y0; yy <= y1; ++yy)
                for (uint32_t xx = x0; xx <= x1; ++xx) {
                    const uint32_t q = yy * R.width + xx, nq = R.count[q];
                    if (nq == 0u)
                        continue;
                    V3 Cq, dq;
                    dn_signal(R, F, q, nq, F.hits[q], demod != 0, Cq, dq);
                    sum = sum + dn_noise(R, q, nq, Cq, dq);
                    ++cnt;
                }
            sig = RtF4{L0.x, L0.y, L0.z, 0.f};
            dn = RtF4{den.x, den.y, den.z, 0.f};
            g0 = RtF4{N.x, N.y, N.z, Z};
            g1 = RtF4{sum / (float)cnt, __uint_as_float(DN_VALID | (h != 0u ? DN_HIT : 0u)), 0.f, 0.f};
        }
        D.sig[0][p] = sig;
        D.den[p] = dn;
        D.guide[2ull * p] = g0;
        D.guide[2ull * p + 1] = g1;
    }
}

struct DnIter {
    const RtF4 *in;
    RtF4 *out;
    const RtF4 *den, *guide;
    float *fb; // the last iteration: L^K * den goes here (3 floats per pixel)
    uint32_t width, height, tiles_x;
    uint32_t stride, sharpness;
    float sigma_color, sigma_depth, inv_stride;
};

DEV float dn_k(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// One pixel of one iteration. tap(dx, dy, L, g0, g1) fetches the records of tap p + stride * (dx, dy) and returns false when it lies outside
// the image; the caller supplies the centre's records.
template <class Tap> DEV V3 dn_pixel(const DnIter &P, const RtF4 Lp, const RtF4 g0p, const RtF4 g1p, Tap tap) {
    const bool hit_p = (__float_as_uint(g1p.y) & DN_HIT) != 0u;
    const float cden = (P.sigma_color * g1p.x) * P.inv_stride + 1e-6f;
    const float pp = (g0p.x * g0p.x + g0p.y * g0p.y) + g0p.z * g0p.z;
    float sw = 0.0f;
    V3 acc = mk(0.f, 0.f, 0.f);
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            RtF4 Lq, g0q, g1q;
            if (!tap(dx, dy, Lq, g0q, g1q))
                continue;
            const uint32_t fq = __float_as_uint(g1q.y);
            if ((fq & DN_VALID) == 0u)
                continue;
            float w = dn_k(dy) * dn_k(dx);
            if (dx != 0 || dy != 0) {
                float wn;
                {
                    const float a = (g0p.x * g0q.x + g0p.y * g0q.y) + g0p.z * g0q.z;
                    const float qq = (g0q.x * g0q.x + g0q.y * g0q.y) + g0q.z * g0q.z;
                    const float pq = pp * qq;
                    if (pp == 0.0f && qq == 0.0f) {
                        wn = 1.0f;
                    } else if (a <= 0.0f || pq == 0.0f) {
                        wn = 0.0f;
                    } else {
                        float c = (a * a) / pq;
                        for (uint32_t j = 0; j < P.sharpness; ++j)
                            c = c * c;
                        wn = c;
                    }
                }
                float wz;
                {
                    const bool hit_q = (fq & DN_HIT) != 0u;
                    if (!hit_p && !hit_q) {
                        wz = 1.0f;
                    } else if (hit_p != hit_q) {
                        wz = 0.0f;
                    } else {
                        const int m = (dx < 0 ? -dx : dx) > (dy < 0 ? -dy : dy) ? (dx < 0 ? -dx : dx) : (dy < 0 ? -dy : dy);
                        const float dist = (float)(P.stride * (uint32_t)m);
                        const float r = (g0p.w - g0q.w) / ((P.sigma_depth * dist) * fmaxf(g0p.w, g0q.w));
                        wz = 1.0f / (1.0f + r * r);
                    }
                }
                const float e = ((fabsf(Lp.x - Lq.x) + fabsf(Lp.y - Lq.y)) + fabsf(Lp.z - Lq.z)) / cden;
                const float wc = 1.0f / (1.0f + e * e);
                w = ((w * wn) * wz) * wc;
            }
            sw = sw + w;
            acc = mk(acc.x + w * Lq.x, acc.y + w * Lq.y, acc.z + w * Lq.z);
        }
    }
    return mk(acc.x / sw, acc.y / sw, acc.z / sw);
}

DEV void dn_store(const DnIter &P, uint32_t p, bool valid, V3 L) {
    if (!valid)
        L = mk(0.f, 0.f, 0.f);
    P.out[p] = RtF4{L.x, L.y, L.z, 0.f};
    if (P.fb) {
        V3 o = mk(0.f, 0.f, 0.f);
        if (valid) {
            const RtF4 d = P.den[p];
            o = mk(L.x * d.x, L.y * d.y, L.z * d.z);
        }
        P.fb[3ull * p] = o.x, P.fb[3ull * p + 1] = o.y, P.fb[3ull * p + 2] = o.z;
    }
}

// T = 1, 2: stride T through an LDS tile of (16 + 4T)^2 records; T = 0: any stride, gathers.
template <int T> __global__ __launch_bounds__(256) void denoise_iter(const DnIter P) {
    constexpr int HALO = 2 * T, TD = DN_TILE + 2 * HALO;
    __shared__ RtF4 s_L[T ? TD * TD : 1], s_g0[T ? TD * TD : 1], s_g1[T ? TD * TD : 1];
    const int bx = (int)(blockIdx.x % P.tiles_x) * DN_TILE, by = (int)(blockIdx.x / P.tiles_x) * DN_TILE;
    const int lx = (int)(threadIdx.x % DN_TILE), ly = (int)(threadIdx.x / DN_TILE);
    const int x = bx + lx, y = by + ly;
    const int W = (int)P.width, H = (int)P.height;
    if constexpr (T != 0) {
        for (int i = (int)threadIdx.x; i < TD * TD; i += 256) {
            const int gx = bx - HALO + i % TD, gy = by - HALO + i / TD;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const uint32_t q = (uint32_t)gy * P.width + (uint32_t)gx;
                s_L[i] = P.in[q], s_g0[i] = P.guide[2ull * q], s_g1[i] = P.guide[2ull * q + 1];
            } else { // outside the image: not valid
                s_L[i] = s_g0[i] = s_g1[i] = RtF4{0.f, 0.f, 0.f, 0.f};
            }
        }
        __syncthreads();
    }
    if (x >= W || y >= H)
        return;
    const uint32_t p = (uint32_t)y * P.width + (uint32_t)x;
    RtF4 Lp, g0p, g1p;
    if constexpr (T != 0) {
        const int c = (ly + HALO) * TD + lx + HALO;
        Lp = s_L[c], g0p = s_g0[c], g1p = s_g1[c];
    } else {
        Lp = P.in[p], g0p = P.guide[2ull * p], g1p = P.guide[2ull * p + 1];
    }
    if ((__float_as_uint(g1p.y) & DN_VALID) == 0u) {
        dn_store(P, p, false, mk(0.f, 0.f, 0.f));
        return;
    }
    V3 L;
    if constexpr (T != 0) {
        L = dn_pixel(P, Lp, g0p, g1p, [&](int dx, int dy, RtF4 &Lq, RtF4 &g0q, RtF4 &g1q) {
            const int c = (ly + HALO + T * dy) * TD + lx + HALO + T * dx; // inside the tile: |T * d| <= HALO
            Lq = s_L[c], g0q = s_g0[c], g1q = s_g1[c];
            return true; // a record from outside the image is marked invalid
        });
    } else {
        const int st = (int)P.stride;
        L = dn_pixel(P, Lp, g0p, g1p, [&](int dx, int dy, RtF4 &Lq, RtF4 &g0q, RtF4 &g1q) {
            const long long qx = (long long)x + (long long)st * dx, qy = (long long)y + (long long)st * dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H)
                return false;
            const uint32_t q = (uint32_t)qy * P.width + (uint32_t)qx;
            Lq = P.in[q], g0q = P.guide[2ull * q], g1q = P.guide[2ull * q + 1];
            return true;
        });
    }
    dn_store(P, p, true, L);
}

} // namespace

namespace rt {

hipError_t launch_denoise(const AccumRound &R, const WfFeat &F, const DenoiseBufs &D, const DenoiseOpt &O, float *fb, hipStream_t stream) {
    const uint64_t n_pix = (uint64_t)R.width * R.height;
    const uint64_t pb = (n_pix + 255u) / 256u;
    hipError_t e = RT_LAUNCH_CHECKED(denoise_prepare, dim3((uint32_t)(pb < 4096u ? pb : 4096u)), dim3(256), 0, stream, R, F, D, O.demodulate ? 1 : 0);
    if (e != hipSuccess)
        return e;
    DnIter P{};
    P.den = D.den, P.guide = D.guide;
    P.width = R.width, P.height = R.height;
    P.tiles_x = (R.width + DN_TILE - 1u) / DN_TILE;
    const uint32_t tiles_y = (R.height + DN_TILE - 1u) / DN_TILE;
    P.sharpness = O.sharpness;
    P.sigma_color = O.sigma_color, P.sigma_depth = O.sigma_depth;
    const dim3 grid(P.tiles_x * tiles_y);
    for (uint32_t i = 0; i < O.iterations; ++i) {
        P.in = D.sig[i & 1u], P.out = D.sig[(i & 1u) ^ 1u];
        P.fb = i + 1u == O.iterations ? fb : nullptr;
        P.stride = 1u << i;
        P.inv_stride = 1.0f / (float)P.stride;
        if (i == 0)
            e = RT_LAUNCH_CHECKED(denoise_iter<1>, grid, dim3(256), 0, stream, P);
        else if (i == 1)
            e = RT_LAUNCH_CHECKED(denoise_iter<2>, grid, dim3(256), 0, stream, P);
        else
            e = RT_LAUNCH_CHECKED(denoise_iter<0>, grid, dim3(256), 0, stream, P);
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace rt
