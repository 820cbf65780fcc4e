// rt_ray_key.h — the ray-order key of the secondary bounces, ONE definition for the kernel that emits it (rt_wf_shade.hip: wf_shade, where it
// makes a ray) and for plain C++ (tests/test_ray_order_key.py compiles a program against it).
//
// 24 bits: the direction octant (3 bits), the Morton code of the origin's cell in a 64^3 grid over the scene bounds (18 bits), then which
// of the octant's sub-cones the direction lies in (3 bits). Rays that start close together and head the same way end up in the same wave of
// wf_extend, so their gathers touch the same nodes (cache lines, L2 residency). Ordering never changes a result: every path's arithmetic is
// independent of where it sits in the queue.
//
// The sub-cone code is (|dx| > |dy|) | (|dy| > |dz|) << 1 | (|dx| > |dz|) << 2. Of its eight values, 3 (x > y > z but not x > z) and 4
// (x > z alone: x <= y <= z) contradict transitivity and only a NaN component can produce 4; 7 is stored as 3. So no key ends in 111, every
// key is below RT_RAY_KEY_PAD, and an entry holding RT_RAY_KEY_PAD sorts strictly behind every ray wherever it stood in the sort's input: the
// ray-order sort runs over the queue's physical positions, unfilled ends of the sub-queue regions included (WfLaunch::emit_keys).
// A NaN component gives a defined key: fmaxf / fminf return their other operand (cell 0), every comparison with it is false.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_KEY_FN __host__ __device__ inline
#else
#define RT_KEY_FN inline
#endif

#define RT_RAY_KEY_BITS 24u
#define RT_RAY_KEY_PAD 0xFFFFFFu /* the RT_RAY_KEY_BITS compared bits of a pad entry (stored as 0xFFFFFFFF: a byte fill) */

RT_KEY_FN uint32_t rt_key_spread3(uint32_t v) { // 6 bits -> every third bit
    v &= 63u;
    v = (v | (v << 8)) & 0x0300Fu;
    v = (v | (v << 4)) & 0x030C3u;
    v = (v | (v << 2)) & 0x09249u;
    return v;
}
RT_KEY_FN uint32_t rt_key_cell(float x, float lo, float inv) { return (uint32_t)fminf(fmaxf((x - lo) * inv * 64.0f, 0.0f), 63.0f); }
// bounds_lo / bounds_inv: DevScene's (lower corner of the scene bounds, 1 / extent)
RT_KEY_FN uint32_t rt_ray_order_key(float ox, float oy, float oz, float dx, float dy, float dz, const float *bounds_lo, const float *bounds_inv) {
    const uint32_t cx = rt_key_cell(ox, bounds_lo[0], bounds_inv[0]), cy = rt_key_cell(oy, bounds_lo[1], bounds_inv[1]), cz = rt_key_cell(oz, bounds_lo[2], bounds_inv[2]);
    const uint32_t morton = rt_key_spread3(cx) | (rt_key_spread3(cy) << 1) | (rt_key_spread3(cz) << 2);
    const uint32_t oct = (dx < 0.0f ? 1u : 0u) | (dy < 0.0f ? 2u : 0u) | (dz < 0.0f ? 4u : 0u);
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    const uint32_t cone = (ax > ay ? 1u : 0u) | (ay > az ? 2u : 0u) | (ax > az ? 4u : 0u);
    return (oct << 21) | (morton << 3) | (cone == 7u ? 3u : cone);
}
