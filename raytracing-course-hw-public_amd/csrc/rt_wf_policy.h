// rt_wf_policy.h — what the host decides about a wavefront pass, stated once: the grids of its launches, and per bounce whether the queue
// is sorted, whether wf_shade emits the next sort's keys, and over how many positions. Plain C++ without a HIP call: launch_wavefront_pass
// (rt_wavefront.hip) asks, tests/test_wf_policy_host.py enumerates the answers on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>

#include "rt_ray_key.h"

#ifndef RT_SHADE_BLOCKS_PER_CU
#define RT_SHADE_BLOCKS_PER_CU 8 /* grid of the grid-stride kernels (wf_shade, wf_extend_prims) */
#endif

namespace rt {

// ---- grids (every kernel of the wavefront files runs blocks of 256 threads, wf_advance's one wave aside)
// one thread per item: ceil(n / 256) blocks, at least one
inline uint32_t wf_grid_items(uint32_t n) {
    const uint32_t blocks = (n + 255u) / 256u;
    return blocks > 0 ? blocks : 1;
}
// a grid-stride loop over n items: as above, but at most `per_cu` blocks per CU. The arithmetic runs in n's own width (32 or 64 bits).
template <class N> inline uint32_t wf_grid_stride(N n, int num_cus, uint32_t per_cu) {
    const N blocks = (n + 255u) / 256u, cap = (N)((uint32_t)num_cus * per_cu);
    const uint32_t g = (uint32_t)(blocks < cap ? blocks : cap);
    return g > 0 ? g : 1;
}

// ---- the ray-order sort of the secondary bounces
// a queue is sorted when its bound is at least this; a shorter one gets the identity order (wf_sort_keys)
constexpr uint32_t WF_SORT_MIN_RAYS = 4096u;

// positions the sub-queue regions written by a wf_shade over at most `bound` rays can span: whole wave slots (rt_device_types.h, WF_STRIPES)
inline size_t wf_key_span(uint32_t bound) { return ((size_t)bound + 63u) / 64u * 64u; }

// Queue sizes reach the host one bounce LATE (launch_wavefront_pass): the size of the queue entering bounce b is known from bounce b + 1 on.
// The host needs it only as an upper bound; queues only shrink, so the size of queue b - 1 bounds queue b.
struct WfPassPolicy {
    uint32_t paths;       // of the pass: the queue entering bounce 0
    uint32_t ray_depth;   // bounces
    bool sizes_read_back; // the pass reads queue sizes back at all (a sort may follow); without it the pass is queued in one go, unsorted

    // bounce b copies the size of the queue it leaves (queue b + 1) to host word b + 1, for bounce b + 2
    bool records_size(uint32_t b) const { return sizes_read_back && b + 1 < ray_depth; }
    // bounce b waits for host word b - 1 before it launches anything
    bool waits_for_size(uint32_t b) const { return sizes_read_back && b >= 2; }
    // the bound of the queue entering bounce b: the pass's path count at bounces 0 and 1 (and wherever nothing is read back), then the size
    // of queue b - 1; `sizes` (word k = size of queue k) is read only where waits_for_size(b)
    uint32_t bound(uint32_t b, const uint32_t *sizes) const { return waits_for_size(b) ? sizes[b - 1] : paths; }
    // nothing is left: bounce b and everything behind it launch nothing (only a size that was read back can say so)
    bool ends_pass(uint32_t b, uint32_t bound) const { return waits_for_size(b) && bound == 0; }

    bool may_sort(uint32_t bound) const { return sizes_read_back && bound >= WF_SORT_MIN_RAYS; }
    // bounce b >= 1 walks its queue in sorted order (else: the identity order), over sort_span(bound) physical positions
    bool sorted(uint32_t b, uint32_t bound) const { return b >= 1 && may_sort(bound); }
    // Bounce b's wf_shade writes the next bounce's sort input itself (WfLaunch::emit_keys), over a pad fill of pad_span(bound) positions. The
    // next bounce's own bound arrives one bounce late but cannot exceed this one, so the question is whether it MAY be sorted:
    // sorted(b + 1, bound') with bound' <= bound implies emits_keys(b, bound), and its sort_span(bound') <= pad_span(bound).
    bool emits_keys(uint32_t b, uint32_t bound) const { return b + 1 < ray_depth && may_sort(bound); }
    static size_t sort_span(uint32_t bound) { return wf_key_span(bound); }
    static size_t pad_span(uint32_t bound) { return wf_key_span(bound); }
};

} // namespace rt
