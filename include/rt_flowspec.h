/*
 * rt_flowspec.h — motion vectors (rt_accum_attach_flow, rt_abi.h: the rule): the inverse of the sensor models, world point to film
 * coordinates, and the flow of one sample, written once so that the HIP kernel (wf_flow) and the CPU tests evaluate the same IEEE-754
 * operation sequence (like rt_devspec.h and rt_primspec.h: + - * / and sqrtf on float, comparisons, the restated libm routines;
 * -ffp-contract=off on both compilers). Every line is one line of the rule in rt_abi.h.
 */
#ifndef RT_FLOWSPEC_H
#define RT_FLOWSPEC_H

#include "rt_abi.h"
#include "rt_devspec.h"

/* What proj reads of a sensor: the frame as given and the host's hoisted terms (rt_sensor above: tan_x, tan_y, half_fov, half_h). */
typedef struct rt_flow_view {
    float P[3], R[3], U[3], F[3];
    float tan_x, tan_y;
    float half_fov;
    float half_width, half_h;
    uint32_t kind; /* RT_SENSOR_* */
} rt_flow_view;

RT_HD float rt_flow_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

RT_HD int rt_flow_finite(float x) { return (rt_f2u(x) & 0x7f800000u) != 0x7f800000u; }

/* X = (V0 * ((1 - b) - c) + V1 * b) + V2 * c, per component: triangle::interop. `v9`: the triangle's nine position floats. */
RT_HD void rt_flow_tri_point(const float v9[9], float b, float c, float X[3]) {
    const float a = (1.0f - b) - c;
    X[0] = (v9[0] * a + v9[3] * b) + v9[6] * c;
    X[1] = (v9[1] * a + v9[4] * b) + v9[7] * c;
    X[2] = (v9[2] * a + v9[5] * b) + v9[8] * c;
}

/* X = o + t * d, per component */
RT_HD void rt_flow_ray_point(const float o[3], const float d[3], float t, float X[3]) {
    X[0] = o[0] + t * d[0];
    X[1] = o[1] + t * d[1];
    X[2] = o[2] + t * d[2];
}

/* proj: film coordinates (fx, fy) of the world point X through `s` at a W x H image; returns ok. Pixel x covers [x, x + 1). Where ok is 0
 * the coordinates are whatever the expressions give (a division by zero included): the caller does not use them. */
RT_HD int rt_flow_proj(const rt_flow_view *s, uint32_t W, uint32_t H, const float X[3], float *fx, float *fy) {
    const float pi_f = 3.14159265358979323846f;
    const float v[3] = {X[0] - s->P[0], X[1] - s->P[1], X[2] - s->P[2]};
    const float r = rt_flow_dot(v, s->R), u = rt_flow_dot(v, s->U), f = rt_flow_dot(v, s->F);
    float nx, ny;
    int ok;
    switch (s->kind) {
    default: /* RT_SENSOR_PINHOLE, RT_SENSOR_THIN_LENS (through the lens centre) */
        ok = f > 0.0f;
        nx = (r / f) / s->tan_x;
        ny = (-(u / f)) / s->tan_y;
        break;
    case RT_SENSOR_ORTHOGRAPHIC:
        ok = f > 0.0f;
        nx = r / s->half_width;
        ny = (-u) / s->half_h;
        break;
    case RT_SENSOR_EQUIRECT: {
        const float len = __builtin_sqrtf((r * r + u * u) + f * f);
        ok = len > 0.0f;
        nx = rt_atan2f_libm(r, f) / pi_f;
        float q = u / len;
        q = q < -1.0f ? -1.0f : (q > 1.0f ? 1.0f : q);
        ny = (-rt_asinf_libm(q)) / (pi_f * 0.5f);
        break;
    }
    case RT_SENSOR_FISHEYE: {
        const float rho = __builtin_sqrtf(r * r + u * u);
        const float th = rt_atan2f_libm(rho, f);
        const float rr = th / s->half_fov;
        if (rho == 0.0f) {
            ok = f > 0.0f;
            nx = 0.0f;
            ny = 0.0f;
        } else {
            ok = 1;
            nx = rr * (r / rho);
            ny = (rr * ((-u) / rho)) / ((float)H / (float)W);
        }
        break;
    }
    }
    *fx = (nx + 1.0f) * (0.5f * (float)W);
    *fy = (ny + 1.0f) * (0.5f * (float)H);
    return ok;
}

/* The flow of a sample that hit: X0 through s0, X1 through s1; returns valid (ok0, ok1, dx and dy finite). EQUIRECT wraps dx once at the seam. */
RT_HD int rt_flow_sample(const rt_flow_view *s0, const rt_flow_view *s1, uint32_t W, uint32_t H, const float X0[3], const float X1[3], float *dx_out, float *dy_out) {
    float fx0, fy0, fx1, fy1;
    const int ok0 = rt_flow_proj(s0, W, H, X0, &fx0, &fy0);
    const int ok1 = rt_flow_proj(s1, W, H, X1, &fx1, &fy1);
    float dx = fx1 - fx0;
    const float dy = fy1 - fy0;
    if (s0->kind == RT_SENSOR_EQUIRECT) {
        if (dx > 0.5f * (float)W)
            dx = dx - (float)W;
        else if (dx < -0.5f * (float)W)
            dx = dx + (float)W;
    }
    *dx_out = dx;
    *dy_out = dy;
    return ok0 && ok1 && rt_flow_finite(dx) && rt_flow_finite(dy);
}

#endif /* RT_FLOWSPEC_H */
