// rt_dev_bake.h — the first ray of a bake sample on the device (rt_abi.h rt_bake): ONE function that makes (origin, direction) of sample S
// of a bake point. The first stage of rt_bake (rt_wf_stages.h WfFromBake), the writer of rt_bake_rays (wf_bake_rays) and the SH resolve
// (wf_resolve_bake, which needs the direction again for the basis) all call it, so sample S of point j is the same ray whoever draws it.
// The rule is stated operation by operation in rt_abi.h; every line here is one line of it.
#pragma once
#include "rt_dev_shade.h"

namespace {

// `p0`, `p1`: the two 16-byte pieces of an rt_bake_point {position, normal.x}, {normal.y, normal.z, stream, reserved}. The direction comes
// from a generator of its own (the thin-lens precedent, rt_dev_sensor.h): the path's stream stays where a camera ray's stands.
// rt_sincos_libm's argument is uniform_real(dg, 0, 2 * PI_F), in [0, 2 pi]: sphere_uniform's own, as wf_shade calls it.
DEV void bake_ray(uint32_t kind, float offset, uint64_t seed, const uint4 &p0, const uint4 &p1, uint32_t S, V3 &o, V3 &d) {
    Rng<RT_RNG_DEVICE> dg;
    rt_xoshiro_seed(&dg.g, seed ^ 0xD6E8FEB86659FD93ull, p1.z, S);
    const V3 v = sphere_uniform(dg);
    const V3 p = mk(__uint_as_float(p0.x), __uint_as_float(p0.y), __uint_as_float(p0.z));
    if (kind == RT_BAKE_SH9) { // the whole sphere around the point: normal and offset are not read
        o = p;
        d = v;
    } else { // RT_BAKE_IRRADIANCE (the host lets no other value through): cosine_dist's lobe, shade_hit's own expression
        const V3 n = mk(__uint_as_float(p0.w), __uint_as_float(p1.x), __uint_as_float(p1.y));
        d = norm(n + v);
        o = p + offset * n;
    }
}

// Y_k(d), k < 9: the real spherical harmonics of bands 0..2 as rt_abi.h lists them
DEV float bake_sh9(uint32_t k, V3 d) {
    switch (k) {
    default:
        return 0.282094792f;
    case 1:
        return 0.488602512f * d.y;
    case 2:
        return 0.488602512f * d.z;
    case 3:
        return 0.488602512f * d.x;
    case 4:
        return 1.092548431f * (d.x * d.y);
    case 5:
        return 1.092548431f * (d.y * d.z);
    case 6:
        return 0.315391565f * (3.0f * (d.z * d.z) - 1.0f);
    case 7:
        return 1.092548431f * (d.x * d.z);
    case 8:
        return 0.546274215f * (d.x * d.x - d.y * d.y);
    }
}

} // namespace
