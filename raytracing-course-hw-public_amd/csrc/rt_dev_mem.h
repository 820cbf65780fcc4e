// rt_dev_mem.h — who owns device memory, and how a failed HIP call is reported (internal; host code of .cpp and .hip files alike).
//
// The only file that calls hipMalloc / hipFree. Two owners:
//   rt::DevArena    a list of allocations with one lifetime: the scratch of a build, the buffers of a scene's geometry, of an environment;
//   rt::DevBuf<T>   one buffer that is grown on demand: framebuffer staging, ray copies, exchange slabs.
// Both are move-only and free in their destructors. Neither synchronises: whoever lets one die (or calls reset()) has made sure that no
// kernel still uses the memory, and that the device it was allocated on is the current one. The device-side builders' scratch makes sure
// itself: it is an rt::ScratchArena (rt_build_host.h), a DevArena that knows its stream and drains it before the frees, on every return path.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rt_abi.h"
#include "rt_error.h"

namespace rt {

// hipError_t -> RT_ERR_*, and the failure "<what>: <HIP's text>" as the entry points report it
inline int hip_code(hipError_t e) { return e == hipErrorOutOfMemory ? RT_ERR_OOM : (e == hipErrorNoDevice ? RT_ERR_NO_DEVICE : RT_ERR_HIP); }
inline int hip_fail(hipError_t e, const std::string &what) { return fail(hip_code(e), what + ": " + hipGetErrorString(e)); }

class DevArena {
  public:
    // `min_bytes`: what a request for nothing allocates, so that every pointer handed out is a real one: that many bytes, or with 0 one
    // element (alloc) / nothing at all and a null pointer (alloc_bytes)
    DevArena() = default;
    explicit DevArena(size_t min_bytes) : min_bytes_(min_bytes) {}
    DevArena(DevArena &&o) noexcept : ptrs_(std::move(o.ptrs_)), min_bytes_(o.min_bytes_) { o.ptrs_.clear(); }
    DevArena &operator=(DevArena &&o) noexcept { // frees what it held; the minimum stays its own
        if (this != &o) {
            reset();
            ptrs_ = std::move(o.ptrs_);
            o.ptrs_.clear();
        }
        return *this;
    }
    DevArena(const DevArena &) = delete;
    DevArena &operator=(const DevArena &) = delete;
    ~DevArena() { reset(); }

    // *p is null after a failure
    template <class T> hipError_t alloc(T **p, size_t count) { return alloc_bytes(p, count ? count * sizeof(T) : (min_bytes_ ? min_bytes_ : sizeof(T))); }
    template <class T> hipError_t alloc_bytes(T **p, size_t bytes) {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, bytes ? bytes : min_bytes_);
        if (e != hipSuccess)
            q = nullptr;
        if (q)
            ptrs_.push_back(q);
        *p = static_cast<T *>(q);
        return e;
    }
    // one allocation leaves: the caller owns `p` from here on (null, or not of this arena: nothing happens)
    template <class T> T *release(T *p) {
        for (size_t k = 0; k < ptrs_.size(); ++k)
            if (ptrs_[k] == static_cast<const void *>(p)) {
                ptrs_.erase(ptrs_.begin() + (std::ptrdiff_t)k);
                break;
            }
        return p;
    }
    // ... and comes in: `p` (from release(), or null) is freed with the rest
    void adopt(const void *p) {
        if (p)
            ptrs_.push_back(const_cast<void *>(p));
    }
    // all of `o` becomes this arena's, behind what it already holds
    void adopt(DevArena &o) {
        ptrs_.insert(ptrs_.end(), o.ptrs_.begin(), o.ptrs_.end());
        o.ptrs_.clear();
    }
    void reset() {
        for (void *p : ptrs_)
            (void)hipFree(p);
        ptrs_.clear();
    }
    bool empty() const { return ptrs_.empty(); }
    size_t size() const { return ptrs_.size(); }

  private:
    std::vector<void *> ptrs_;
    size_t min_bytes_ = 0;
};

template <class T> class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }

    // room for `count` elements. Grow-only; the content does not survive growth: the old block is freed BEFORE the new one is asked for (the
    // two never have to fit side by side), so after a failure the buffer is empty.
    hipError_t reserve(size_t count) {
        if (cap_ >= count)
            return hipSuccess;
        reset();
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, count * sizeof(T));
        if (e != hipSuccess)
            return e;
        p_ = static_cast<T *>(q);
        cap_ = count;
        return hipSuccess;
    }
    void reset() {
        if (p_)
            (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    T *get() const { return p_; }
    size_t capacity() const { return cap_; } // elements

  private:
    T *p_ = nullptr;
    size_t cap_ = 0;
};

} // namespace rt

// in a function that returns RT_ERR_*: a failed call ends it with rt::hip_fail, named by its own text
#define HIP_TRY(expr)                          \
    do {                                       \
        hipError_t e_ = (expr);                \
        if (e_ != hipSuccess)                  \
            return rt::hip_fail(e_, #expr);    \
    } while (0)

// in a function that returns hipError_t and has a `const char **err` (the device-side builders): a failed call ends it with its own text in *err
#define HIP_TRY_ERR(expr)          \
    do {                           \
        hipError_t e_ = (expr);    \
        if (e_ != hipSuccess) {    \
            if (err)               \
                *err = #expr;      \
            return e_;             \
        }                          \
    } while (0)
