// rt_build_host.h — the host steps every device-side builder takes (rt_bvh_device.hip and its stages, rt_wide_pack.hip, rt_wide_refit.hip,
// rt_update_dev.hip), each stated once: the scratch of a build on a stream, the read-back of a few words, the total of an exclusive scan.
// Host only, HIP's runtime API only (internal; rocPRIM's part is rt_build_scan.h).
#pragma once
#include <cstdint>

#include "rt_dev_mem.h"

namespace rt {

// The scratch of a build whose kernels run on `stream`: drains the stream, then frees. Every return path of a builder, the failed ones
// included, so leaves no kernel running on memory about to be freed, nor on the caller's arrays. One type, so there is no guard to declare
// in the right order; on the success path the stream is idle already and the drain costs one call.
class ScratchArena : public DevArena {
  public:
    explicit ScratchArena(hipStream_t stream, size_t min_bytes = 0) : DevArena(min_bytes), stream_(stream) {}
    ~ScratchArena() { (void)hipStreamSynchronize(stream_); } // then ~DevArena frees
    ScratchArena(const ScratchArena &) = delete;
    ScratchArena &operator=(const ScratchArena &) = delete;

  private:
    hipStream_t stream_;
};

// `count` words (or other small records) from the device to `dst`, there when this returns
template <class T> hipError_t read_back(T *dst, const T *src, size_t count, hipStream_t stream) {
    const hipError_t e = hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, stream);
    return e != hipSuccess ? e : hipStreamSynchronize(stream);
}

// The total of an exclusive scan of `n` values (n > 0) is its last offset plus the last value; in 64 bits, since the sum of 32-bit values
// may not fit in 32.
inline uint64_t scan_total(uint32_t last_offset, uint32_t last_value) { return (uint64_t)last_offset + last_value; }
inline hipError_t scan_total(const uint32_t *values, const uint32_t *offsets, size_t n, hipStream_t stream, uint64_t *total) {
    uint32_t last[2] = {0u, 0u};
    hipError_t e = hipMemcpyAsync(&last[0], offsets + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess)
        e = read_back(&last[1], values + (n - 1), 1, stream);
    *total = scan_total(last[0], last[1]);
    return e;
}

} // namespace rt
