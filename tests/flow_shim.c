/* flow_shim.c: include/rt_flowspec.h behind two C functions, so that tests/flow_replay.py can call the very definition the wf_flow kernel is
 * compiled from (the equirect and fisheye projections go through the restated libm routines, which numpy does not have). Compiled by the
 * tests with the host compiler, -O2 -ffp-contract=off. */
#include <stddef.h>

#include "rt_flowspec.h"

void flow_shim_proj(const rt_flow_view *s, uint32_t W, uint32_t H, const float *X, uint32_t n, float *fx, float *fy, int32_t *ok) {
    for (uint32_t i = 0; i < n; ++i)
        ok[i] = rt_flow_proj(s, W, H, X + 3 * (size_t)i, fx + i, fy + i);
}

void flow_shim_sample(const rt_flow_view *s0, const rt_flow_view *s1, uint32_t W, uint32_t H, const float *X0, const float *X1, uint32_t n, float *dx, float *dy,
                      int32_t *valid) {
    for (uint32_t i = 0; i < n; ++i)
        valid[i] = rt_flow_sample(s0, s1, W, H, X0 + 3 * (size_t)i, X1 + 3 * (size_t)i, dx + i, dy + i);
}
