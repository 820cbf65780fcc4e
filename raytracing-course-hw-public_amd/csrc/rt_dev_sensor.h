// rt_dev_sensor.h — the cameras of the wavefront pipeline on the device (rt_abi.h rt_sensor; a view of rt_render* is a pinhole record): ONE
// function that makes (origin, direction, RNG state) of sample s of pixel pix from a sensor record. The camera source of the first
// stage (rt_wf_stages.h WfFromCameras), the list source of the accumulators (WfFromList) and the writer of rt_sensor_rays (wf_sensor_rays) all call it, so sample s of
// pixel p is the same ray whoever draws it. The rule is stated operation by operation in rt_abi.h; every line here is one line of it.
#pragma once
#include "rt_dev_shade.h"

namespace {

// `sn` is the caller's copy of the record: scalar registers where the wave reads one sensor, and then `sn.kind` is a scalar branch.
// rt_sincos_libm arguments (its restatement holds on [0, 2 pi], rt_devspec.h):
//   nx, ny in [-1, 1] as rounded: x + ox <= W and 2 * W / W = 2 exactly; so nx + 1, ny + 1 in [0, 2];
//   EQUIRECT   a = PI_F * (nx + 1) <= PI_F * 2 = (2 * PI_F), an exact doubling; p <= (PI_F * 0.5f) * 2 = PI_F;
//   FISHEYE    th = r * half_fov with half_fov > 0 and half_fov * sqrt(1 + (H/W)^2) <= pi (the host refuses anything else), r within a few
//              ulp of that root: th < 1.000001 * pi;
//   THIN_LENS  (2 * PI_F) * l1 with l1 in [0, 1).
DEV void sensor_ray(const WfSensor &sn, uint32_t width, uint32_t height, uint32_t pix, uint32_t s, V3 &o, V3 &d, Rng<RT_RNG_DEVICE> &rng) {
    const V3 P = ld3(sn.pos), R = ld3(sn.right), U = ld3(sn.up), F = ld3(sn.fwd);
    rt_xoshiro_seed(&rng.g, sn.seed, pix, s);
    float nx, ny;
    gen_ray_film(rng, pix, width, height, nx, ny); // the two jitter draws: `rng` is not touched again
    o = P;
    switch (sn.kind) {
    default: // RT_SENSOR_PINHOLE (the host lets no other value through): gen_ray itself
        d = norm(gen_ray_screen(nx, ny, sn.tan_x, sn.tan_y, R, U, F));
        break;
    case RT_SENSOR_EQUIRECT: {
        const float a = PI_F * (nx + 1);
        const float p = (PI_F * 0.5f) * (ny + 1);
        float sa, ca, sp, cp;
        rt_sincos_libm(a, &sa, &ca);
        rt_sincos_libm(p, &sp, &cp);
        d = norm((-(sp * sa)) * R + cp * U + (-(sp * ca)) * F);
        break;
    }
    case RT_SENSOR_FISHEYE: {
        const float px = nx;
        const float py = ny * ((float)height / (float)width);
        const float r = __builtin_sqrtf(px * px + py * py);
        const float th = r * sn.half_fov;
        float st, ct;
        rt_sincos_libm(th, &st, &ct);
        const V3 off = (st * (px / r)) * R - (st * (py / r)) * U + ct * F;
        d = norm(r == 0.0f ? F : off);
        break;
    }
    case RT_SENSOR_ORTHOGRAPHIC:
        o = P + (nx * sn.half_width) * R - (ny * sn.half_h) * U;
        d = norm(F);
        break;
    case RT_SENSOR_THIN_LENS: {
        const V3 q = gen_ray_screen(nx, ny, sn.tan_x, sn.tan_y, R, U, F);
        Rng<RT_RNG_DEVICE> lens;
        rt_xoshiro_seed(&lens.g, sn.seed ^ 0x9E3779B97F4A7C15ull, pix, s);
        const float l0 = uniform_real(lens, 0.0f, 1.0f);
        const float l1 = uniform_real(lens, 0.0f, 1.0f);
        const float rad = sn.lens_radius * __builtin_sqrtf(l0);
        float sl, cl;
        rt_sincos_libm((2 * PI_F) * l1, &sl, &cl);
        const V3 e = (rad * cl) * R + (rad * sl) * U;
        o = P + e;
        d = norm(sn.focus_distance * q - e);
        break;
    }
    }
}

// The sensor of a lane: wave-uniform except where a wave straddles two sensors of a multi-sensor call. The uniform wave reads the record
// through scalar loads and branches on a scalar kind; the straddling wave reads per lane. `emit(o, d, rng)`.
template <class Emit> DEV void sensor_ray_of(const WfSensor *table, uint32_t v, uint32_t width, uint32_t height, uint32_t pix, uint32_t s, Emit emit) {
    const uint32_t v0 = __builtin_amdgcn_readfirstlane(v);
    V3 o, d;
    Rng<RT_RNG_DEVICE> rng;
    if (__ballot(v != v0) == 0ull)
        sensor_ray(table[v0], width, height, pix, s, o, d, rng);
    else
        sensor_ray(table[v], width, height, pix, s, o, d, rng);
    emit(o, d, rng);
}

} // namespace
