// rt_dev_env.h — the float environment of rt_set_environment (rt_abi.h states the rule): its radiance lookup, the solid-angle pdf of its
// piecewise-constant distribution and the sampler. The one definition of each: shade_hit, bg_at and the probes (rt_bg_at, rt_env_pdf,
// rt_env_sample) all call these.
#pragma once
#include "rt_dev_surface.h"

namespace {

// What the miss branch looks up and whether mix_dist has the environment as a component: shade_hit's and bg_at's template value.
// NONE and TEX8 are the two kinds the reference has (the constant background; Scene::bg as an 8-bit texture with gamma).
enum { ENV_NONE = 0, ENV_TEX8 = 1, ENV_FLOAT = 2, ENV_FLOAT_DIST = 3 };

// Texture::sample's addressing for the direction's (u, v) = rt_bg_uv(dir): the texel (x0, y0) of the footprint names the cell.
DEV TexFoot env_foot(const DevEnv &E, V3 dir) {
    float u, v;
    rt_bg_uv(dir.x, dir.y, dir.z, &u, &v);
    DevTexture T{};
    T.width = E.width, T.height = E.height;
    return TexFoot(T, u, v);
}

// Le(dir) = bg_color * env(u, v): tex_sample's footprint, wrap and bilinear weights over float texels, no decode and no gamma. A 1x1 map
// returns its texel before looking at the direction, like Texture::sample's 1x1 path.
template <bool STATS> DEV V3 env_radiance(const DevScene &S, V3 dir, LaneStats<STATS> &st) {
    const DevEnv &E = S.env;
    const float4 *tx = reinterpret_cast<const float4 *>(E.texels);
    if (E.width * E.height == 1u) {
        const float4 t = tx[0];
        return ld3(S.bg) * mk(t.x, t.y, t.z);
    }
    const TexFoot F = env_foot(E, dir);
    const Tex4<float4> q = F.fetch([&](int x, int y) { return tx[(size_t)(uint32_t)y * E.width + (uint32_t)x]; });
    st.texels(4);
    auto c4 = [](float4 t) { return C4{t.x, t.y, t.z, t.w}; };
    const C4 c = (1 - F.dx) * ((1 - F.dy) * c4(q.q00) + F.dy * c4(q.q01)) + F.dx * ((1 - F.dy) * c4(q.q10) + F.dy * c4(q.q11));
    return ld3(S.bg) * mk(c.r, c.g, c.b);
}

// The cell (row i, column j) of a direction: the footprint's first texel, clamped for memory safety only (a NaN direction lands in some cell)
DEV void env_cell(const DevEnv &E, V3 dir, uint32_t &i, uint32_t &j) {
    const TexFoot F = env_foot(E, dir);
    i = (uint32_t)F.y0 < E.height ? (uint32_t)F.y0 : E.height - 1u;
    j = (uint32_t)F.x0 < E.width ? (uint32_t)F.x0 : E.width - 1u;
}

// pdf(dir) = p_ij / Omega_ij from the stored float tables: p_ij = (marg[i + 1] - marg[i]) * (row_i[j + 1] - row_i[j])
DEV float env_pdf(const DevEnv &E, V3 dir) {
    uint32_t i, j;
    env_cell(E, dir, i, j);
    const float *row = E.rows + (size_t)i * (E.width + 1u);
    const float pm = E.marg[i + 1u] - E.marg[i];
    const float pr = row[j + 1u] - row[j];
    return (pm * pr) / E.band[E.height + 1u + i];
}

// the last k in [0, n) with cdf[k] <= x (cdf[0] = 0 and cdf[n] = 1 > x: cell k has cdf[k] <= x < cdf[k + 1], never an empty one)
DEV uint32_t env_search(const float *cdf, uint32_t n, float x) {
    uint32_t lo = 0u, hi = n - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (cdf[mid] <= x)
            lo = mid;
        else
            hi = mid - 1u;
    }
    return lo;
}

// The direction of four uniforms in [0, 1): row by x0, column by x1, then uniform in solid angle inside the cell. It inverts rt_bg_uv.
DEV V3 env_sample_xi(const DevEnv &E, float x0, float x1, float x2, float x3) {
    const uint32_t i = env_search(E.marg, E.height, x0);
    const uint32_t j = env_search(E.rows + (size_t)i * (E.width + 1u), E.width, x1);
    const float u = ((float)j + x2) / (float)E.width;
    const float ct = E.band[i], cb = E.band[i + 1u];
    const float dy = ct - x3 * (ct - cb);
    const float r = __builtin_sqrtf(rmax(0.0f, 1 - dy * dy));
    float s, c;
    rt_sincos_libm((2.0f * PI_F) * u, &s, &c);
    return {-(r * c), dy, -(r * s)};
}
template <class R> DEV V3 env_sample(const DevEnv &E, R &rng) {
    const float x0 = uniform_real(rng, 0.0f, 1.0f);
    const float x1 = uniform_real(rng, 0.0f, 1.0f);
    const float x2 = uniform_real(rng, 0.0f, 1.0f);
    const float x3 = uniform_real(rng, 0.0f, 1.0f);
    return env_sample_xi(E, x0, x1, x2, x3);
}

} // namespace
