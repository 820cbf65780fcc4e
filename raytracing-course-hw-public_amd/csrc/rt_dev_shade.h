// rt_dev_shade.h — one shade() level: primary-ray generation, the sampling distributions, the BRDF, the background and shade_hit.
#pragma once
#include "rt_dev_env.h"

namespace {

// gen_ray (raytracer.h:527-538): the two jitter draws, the screen position and the normalised direction of a sample of pixel `pix`, with the
// tangents hoisted. The megakernel and the wavefront pipeline both call this, so their primary rays are the same operation sequence.
// In three steps, each with one definition, because the sensor models (rt_dev_sensor.h) share the first with every kind and the second with
// the thin lens: the jittered film position in [-1, 1]^2, the screen point in front of the camera, its normalisation.
template <class R> DEV void gen_ray_film(R &rng, uint32_t pix, uint32_t width, uint32_t height, float &nx, float &ny) {
    const uint32_t x = pix % width, y = pix / width;
    float ox = uniform_real(rng, 0.0f, 1.0f);
    float oy = uniform_real(rng, 0.0f, 1.0f);
    nx = 2 * ((float)(int)x + ox) / (float)width - 1;
    ny = 2 * ((float)(int)y + oy) / (float)height - 1;
}
DEV V3 gen_ray_screen(float nx, float ny, float tan_x, float tan_y, V3 cam_right, V3 cam_up, V3 cam_fwd) {
    float sx = nx * tan_x;
    float sy = ny * tan_y;
    return sx * cam_right - sy * cam_up + 1.0f * cam_fwd;
}
template <class R> DEV V3 gen_ray_dir(R &rng, uint32_t pix, uint32_t width, uint32_t height, float tan_x, float tan_y, V3 cam_right, V3 cam_up, V3 cam_fwd) {
    float nx, ny;
    gen_ray_film(rng, pix, width, height, nx, ny);
    return norm(gen_ray_screen(nx, ny, tan_x, tan_y, cam_right, cam_up, cam_fwd));
}

// ---------------------------------------------------------------------------------------------- sampling + BRDF
template <class R> DEV V3 sphere_uniform(R &rng) { // raytracer.h:94-105
    float z = uniform_real(rng, -1.0f, 1.0f);
    float co_z = __builtin_sqrtf(rmax(0.0f, 1 - z * z));
    float phi = uniform_real(rng, 0.0f, 2 * PI_F);
    float s, c;
    rt_sincos_libm(phi, &s, &c); // std::cos / std::sin on floats = glibc cosf / sinf, restated bit for bit (rt_devspec.h)
    return {co_z * c, co_z * s, z};
}
DEV V3 halfway(V3 in_dir, V3 out_dir) { return norm(out_dir - in_dir); } // :131-134
DEV V3 choose_local_x(V3 n) { // :208-219
    V3 res{1, 1, 1};
    if (__builtin_fabsf(n.x) > 0.5f)
        res.x -= dot(res, n) / n.x;
    else if (__builtin_fabsf(n.y) > 0.5f)
        res.y -= dot(res, n) / n.y;
    else
        res.z -= dot(res, n) / n.z;
    return norm(res);
}
template <class R> DEV V3 vndf_sample(R &rng, float roughness, V3 in_dir, V3 normal) { // :140-173
    V3 nx = choose_local_x(normal);
    V3 ny = crs(normal, nx);
    V3 v = -norm(mk(dot(nx, in_dir), dot(ny, in_dir), dot(normal, in_dir)));
    V3 vh = norm(mk(roughness, roughness, 1) * v);
    float lensq = vh.x * vh.x + vh.y * vh.y;
    V3 T1 = lensq > 0 ? mk(-vh.y, vh.x, 0) / __builtin_sqrtf(lensq) : mk(1, 0, 0);
    V3 T2 = crs(vh, T1);
    float r = __builtin_sqrtf(uniform_real(rng, 0, 1));
    float phi = 2.0f * PI_F * uniform_real(rng, 0, 1);
    float sn, cs;
    rt_sincos_libm(phi, &sn, &cs);
    float t1 = r * cs;
    float t2 = r * sn;
    float s = 0.5f * (1.0f + vh.z);
    t2 = (1.0f - s) * __builtin_sqrtf(1.0f - pow2(t1)) + s * t2;
    V3 nh = transform3(mk(t1, t2, __builtin_sqrtf(rmax(0.0f, 1.0f - pow2(t1) - pow2(t2)))), T1, T2, vh);
    V3 ne = norm(mk(roughness * nh.x, roughness * nh.y, rmax(0.0f, nh.z)));
    V3 res_n = norm(transform3(ne, nx, ny, normal));
    return in_dir - 2 * res_n * dot(in_dir, res_n); // reflect geometry.h:36-40
}
DEV float vndf_pdf(float roughness, V3 in_dir, V3 normal, V3 dir) { // :175-206
    V3 nx = choose_local_x(normal);
    V3 ny = crs(normal, nx);
    V3 v = -mk(dot(nx, in_dir), dot(ny, in_dir), dot(normal, in_dir));
    V3 nv = halfway(in_dir, dir);
    V3 n = mk(dot(nx, nv), dot(ny, nv), dot(normal, nv));
    float vdn = dot(v, n);
    if (vdn <= 0)
        return 0;
    float vx = v.x * roughness, vy = v.y * roughness;
    float lambda = (-1 + __builtin_sqrtf(1 + (vx * vx + vy * vy) / pow2(v.z))) / 2;
    float g1 = 1 / (1 + lambda);
    float dn = 1 / PI_F / roughness / roughness / pow2(len2(n / mk(roughness, roughness, 1)));
    float dv = g1 * vdn * dn / rmax(EPS, v.z);
    return dv / 4 / vdn;
}
DEV float heaviside(float x) { return x > 0 ? 1.0f : 0.0f; }
DEV float specular_brdf(float alpha, V3 in_dir, V3 out_dir, V3 normal) { // :273-293
    V3 h = halfway(in_dir, out_dir);
    float ndh = dot(normal, h);
    float d = pow2(alpha) * heaviside(ndh) / PI_F / pow2(pow2(ndh) * (pow2(alpha) - 1) + 1);
    float ndo = dot(normal, out_dir);
    float ndi = dot(normal, -in_dir);
    float div1 = (__builtin_fabsf(ndo) + __builtin_sqrtf(pow2(alpha) + (1 - pow2(alpha)) * pow2(ndo)));
    float div2 = (__builtin_fabsf(ndi) + __builtin_sqrtf(pow2(alpha) + (1 - pow2(alpha)) * pow2(ndi)));
    float v = heaviside(dot(h, out_dir)) * heaviside(dot(h, -in_dir)) / div1 / div2;
    return v * d;
}
DEV V3 pbr_brdf(V3 in_dir, V3 out_dir, const Surf &ii) { // :300-343
    V3 res{0, 0, 0};
    V3 base = mk(ii.color.r, ii.color.g, ii.color.b);
    float alpha = pow2(rmax(ii.roughness, MIN_ROUGHNESS));
    float sp = specular_brdf(alpha, in_dir, out_dir, ii.shading_normal);
    V3 spec = mk(sp, sp, sp);
    float VdotH = dot(-in_dir, halfway(in_dir, out_dir));
    float fw = pow5(1 - __builtin_fabsf(VdotH));
    if (ii.metallic < 1) {
        V3 diffuse = base / PI_F;
        float f0 = pow2((1 - ii.ior) / (1 + ii.ior));
        float fr = f0 + (1 - f0) * fw;
        V3 dielectric = diffuse * (1 - fr) + spec * fr;
        res = res + (1 - ii.metallic) * dielectric;
    }
    if (ii.metallic > 0) {
        V3 metal = spec * (base + (1 - base) * fw);
        res = res + ii.metallic * metal;
    }
    return res;
}

// Scene::bg_at (scene.h:83-89): bg_color * bg.sample({x, y}, 2.2f).rgb(). With the default 1x1 WHITE_TEXTURE (USE_ENV_MAP = false,
// config.h:37) Texture::sample returns its only texel before looking at the coordinates, so nothing is evaluated. With an environment
// map the direction goes through the reference's own atan2f / asinf (rt_devspec.h rt_bg_uv) and the ordinary texture lookup with gamma.
// ENV (rt_dev_env.h) = ENV_NONE compiles the lookup out (wf_shade's default instantiations keep their register budget; the launcher picks
// ENV by scene). ENV_FLOAT / ENV_FLOAT_DIST: the float map of rt_set_environment takes the texture's place (env_radiance).
template <bool STATS, int ENV = ENV_TEX8> DEV V3 bg_at(const DevScene &S, V3 dir, const float *s_lin, const float *s_gam, LaneStats<STATS> &st) {
    if constexpr (ENV == ENV_FLOAT || ENV == ENV_FLOAT_DIST)
        return env_radiance<STATS>(S, dir, st);
    if (ENV == ENV_NONE || S.bg_tex < 0)
        return ld3(S.bg) * mk(1, 1, 1);
    float u, v;
    rt_bg_uv(dir.x, dir.y, dir.z, &u, &v);
    const C4 c = tex_sample<STATS>(S, S.bg_tex, TEX_DEFAULT_WHITE, u, v, true, s_lin, s_gam, st);
    return ld3(S.bg) * mk(c.r, c.g, c.b);
}

// ---------------------------------------------------------------------------------------------- one shade() level
// trace_ray's hit / miss branch (raytracer.h:602-604) + shade (raytracer.h:555-591) for ONE cast result, without the
// recursion: the caller owns depth bookkeeping and the (emission, scale) fold stack.
//   terminal : the path ends here and contributes `term` to the innermost pending frame
//   push     : a scattering event happened: push (emission, scl) and continue with the ray (nro, nrd)
//   neither  : stochastic alpha pass-through (:559-561): continue with (nro, nrd), no frame
// RNG draw order is the reference's: alpha coin, technique coin, then the sampler's own draws.
// Which sampler the NEXT shade() of a path will run, from the generator state the path record stores (taken by value): the alpha coin
// is drawn first whatever the material (:559), the technique coin second (:565), mix_dist's pick third (:386). 0 VNDF, 1 cosine, 2 light
// triangle. A scheduling hint for wf_shade's lane assignment only: a miss or an alpha pass-through never gets that far, and nothing
// computed depends on it. ENV_DIST: mix_dist has the environment as its last component (ENV_FLOAT_DIST); its sampler is handed out with
// class 2: two dependent binary searches through the tables in HBM cost what the light sampler's record fetch costs, not what the
// arithmetic-only cosine lobe does, and in a scene without emissive triangles class 2 is otherwise empty.
template <bool ENV_DIST = false, class R> DEV uint32_t next_shade_class(R rng, bool has_lights) {
    (void)uniform_real(rng, 0.0f, 1.0f);
    if (uniform_real(rng, 0.0f, 1.0f) <= VNDF_FACTOR)
        return 0u;
    if constexpr (ENV_DIST)
        return rng.below(has_lights ? 3u : 2u) == 0u ? 1u : 2u;
    return (!has_lights || rng.below(2) == 0u) ? 1u : 2u;
}
// bvh_mix_dist::sample :353-361 + triangle_dist::sample :225-239: a uniformly picked light triangle, a uniform point on it
template <class R> DEV V3 light_sample(const DevScene &S, const LightTabs &LT, V3 pos, R &rng) {
    const uint32_t id = rng.below(S.lights.n_tris);
    const float4 *lp = LT.tris + 3u * id;
    const TriRec lt = tri_rec(lp[0], lp[1], lp[2]);
    float u = uniform_real(rng, 0, 1);
    float v = uniform_real(rng, 0, 1);
    if (u + v > 1) {
        u = 1 - u;
        v = 1 - v;
    }
    V3 p = lt.a + lt.v * v + lt.u * u; // a + v' * v + u' * u
    return norm(p - pos);
}
struct ShadeResult {
    bool terminal, push;
    V3 term, emission, scl, nro, nrd;
};
template <class R, bool STATS, int ENV = ENV_TEX8, class STK>
DEV ShadeResult shade_hit(const DevScene &S, const LightTabs &LT, const Hit &h, V3 ro, V3 rd, R &rng, bool has_lights, STK &stk, const float *s_lin,
                          const float *s_gam, LaneStats<STATS> &st) {
    ShadeResult out;
    out.terminal = false;
    out.push = false;
    out.term = out.emission = out.scl = out.nro = mk(0, 0, 0);
    out.nrd = mk(0, 0, 1);
    if (h.k == RT_NONE) {
        out.terminal = true;
        out.term = bg_at<STATS, ENV>(S, rd, s_lin, s_gam, st);
        return out;
    }
    const Surf ii = make_surf<STATS>(S, h, ro, rd, s_lin, s_gam, st);
    const V3 pos = ro + rd * h.t;                          // ray.at(t)
    if (!(uniform_real(rng, 0.0f, 1.0f) <= ii.color.a)) { // !coin(alpha) :559-561
        out.nro = pos;
        out.nrd = rd;
        return out;
    }
    const float vr = pow2(rmax(ii.roughness, MIN_ROUGHNESS)); // :563-564
    V3 dir;
    constexpr bool ENV_DIST = ENV == ENV_FLOAT_DIST; // mix_dist gains the environment as one more equally weighted component
    const uint32_t mix_k = has_lights ? 3u : 2u;     // ... {cosine, lights, env} or {cosine, env}
    if (uniform_real(rng, 0.0f, 1.0f) <= VNDF_FACTOR) { // :565
        dir = vndf_sample(rng, vr, rd, ii.shading_normal);
    } else if (ENV_DIST) {
        const uint32_t pick = rng.below(mix_k);
        if (pick == 0) {
            dir = norm(ii.normal + sphere_uniform(rng));
        } else if (pick + 1u == mix_k) {
            dir = env_sample(S.env, rng);
        } else {
            dir = light_sample(S, LT, pos, rng);
        }
    } else if (!has_lights) { // dir_dist = cosine_dist (:449)
        dir = norm(ii.normal + sphere_uniform(rng));
    } else { // mix_dist{cosine, bvh_mix} (:381-393)
        const uint32_t pick = rng.below(2);
        if (pick == 0) {
            dir = norm(ii.normal + sphere_uniform(rng));
        } else {
            dir = light_sample(S, LT, pos, rng);
        }
    }
    if (isnan_f(dir.x) || isnan_f(dir.y) || isnan_f(dir.z)) { // :569-571
        out.terminal = true;
        out.term = ii.emission;
        return out;
    }
    const float VNDF_p = vndf_pdf(vr, rd, ii.shading_normal, dir);
    float MIS_p;
    const float cos_p = rmax(dot(ii.normal, dir) / PI_F, 0.0f); // cosine_dist::pdf :123-128
    if (ENV_DIST) { // mix_dist::pdf over k components: (sum of the component pdfs) / k
        float r = 0;
        r += cos_p;
        if (has_lights)
            r += lights_pdf<STATS>(S, LT, pos, dir, stk, st);
        r += env_pdf(S.env, dir);
        MIS_p = r / (float)mix_k;
    } else if (!has_lights) {
        MIS_p = cos_p;
    } else { // mix_dist::pdf :395-407
        float r = 0;
        r += cos_p;
        r += lights_pdf<STATS>(S, LT, pos, dir, stk, st);
        MIS_p = r / 2.0f;
    }
    const float p = VNDF_FACTOR * VNDF_p + (1 - VNDF_FACTOR) * MIS_p;
    if (p < EPS) { // :576-578
        out.terminal = true;
        out.term = ii.emission;
        return out;
    }
    const V3 scl = pbr_brdf(rd, dir, ii) / p * rmax(0.0f, dot(dir, ii.shading_normal));
    if (len2(scl) == 0.0f) { // :584-586
        out.terminal = true;
        out.term = ii.emission;
        return out;
    }
    out.push = true;
    out.emission = ii.emission;
    out.scl = scl;
    out.nro = pos;
    out.nrd = dir;
    return out;
}

} // namespace
