// rt_call_io.h — the arrays of one call of an entry point: taken from the host or, with RT_FLAG_DEVICE_FB, from the caller's HBM (internal).
//
// An entry point DECLARES its arrays on an rt::CallIo (in / out / out_ranges / scratch: each names the pointer variable its kernels will
// use), then runs: reserve() sizes ONE block of the staging owner for everything that has to be staged and only then fills the pointer
// variables in (DevBuf::reserve frees on growth: no pointer into the block exists before it); upload() queues the host inputs, download()
// the copies back to host destinations; run() is reserve, then queue_and_wait over upload, the caller's launches and download. Nothing here
// synchronises or queues outside queue_and_wait, the one implementation of "no return with work in flight".
//   caller's arrays in HBM   an input or output is the caller's pointer, untouched (null stays null); only scratch is staged
//   host call                every array is a region of the block, 256-byte aligned; a null destination is computed and not copied
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <type_traits>
#include <vector>

#include "rt_dev_mem.h"

namespace rt {

// Everything `queue` puts on `stream` has finished when this returns: a failure in between must not return while kernels or copies are
// still in flight (a later reservation or rt_destroy would free memory under them; a caller may release its host arrays)
template <class Queue> int queue_and_wait(hipStream_t stream, Queue queue) {
    if (int rc = queue(); rc != RT_OK) {
        (void)hipStreamSynchronize(stream);
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return RT_OK;
}

class CallIo {
  public:
    // `staging`: grow-only, of the scene or of the call; `device`: the caller's arrays are in HBM
    CallIo(hipStream_t stream, DevBuf<uint8_t> &staging, bool device) : stream_(stream), staging_(staging), device_(device) {}
    CallIo(const CallIo &) = delete; // the pointer variables it names are one call's

    // what the kernels read: *d is the caller's array, or its staged copy (upload)
    template <class T> void in(const T **d, std::type_identity_t<const T *> caller, size_t bytes) {
        const size_t r = add(d, caller, bytes, !device_);
        if (!device_ && bytes)
            ups_.push_back({r, 0, bytes});
    }
    // what the kernels write: *d is the caller's array, or a region that download copies to a non-null host destination
    template <class T> void out(T **d, std::type_identity_t<T *> caller, size_t bytes) { range(out_ranges(d, caller, bytes), 0, bytes); }
    // ... of which only the byte ranges named afterwards come back (a shard's blocks; a count known after a first run)
    template <class T> size_t out_ranges(T **d, std::type_identity_t<T *> caller, size_t bytes) { return add(d, caller, bytes, !device_); }
    void range(size_t region, size_t first, size_t bytes) {
        if (regions_[region].staged && regions_[region].caller && bytes)
            downs_.push_back({region, first, bytes});
    }
    // internal also when the caller's arrays are in HBM: the float image behind an rgb8 destination, a kernel's workspace
    template <class T> void scratch(T **d, size_t bytes) { add(d, nullptr, bytes, true); }

    int reserve() {
        HIP_TRY(staging_.reserve(total_));
        for (const Region &r : regions_)
            r.set(r.slot, r.staged ? staging_.get() + r.offset : r.caller);
        return RT_OK;
    }
    int upload() {
        for (const Copy &c : ups_)
            HIP_TRY(hipMemcpyAsync(staged(c), host(c), c.bytes, hipMemcpyHostToDevice, stream_));
        return RT_OK;
    }
    int download() {
        for (const Copy &c : downs_)
            HIP_TRY(hipMemcpyAsync(host(c), staged(c), c.bytes, hipMemcpyDeviceToHost, stream_));
        return RT_OK;
    }
    template <class Body> int run(Body body) {
        if (int rc = reserve(); rc != RT_OK)
            return rc;
        return queue_and_wait(stream_, [&]() -> int {
            if (int rc = upload(); rc != RT_OK)
                return rc;
            if (int rc = body(); rc != RT_OK)
                return rc;
            return download();
        });
    }

  private:
    struct Region {
        size_t offset;
        void *slot;                       // the entry point's pointer variable ...
        void (*set)(void *slot, void *p); // ... and how to assign to it
        void *caller;
        bool staged;
    };
    struct Copy {
        size_t region, first, bytes;
    };
    template <class T> size_t add(T **d, const void *caller, size_t bytes, bool staged) {
        *d = nullptr;
        regions_.push_back({total_, d, [](void *slot, void *p) { *static_cast<T **>(slot) = static_cast<T *>(p); }, const_cast<void *>(caller), staged});
        if (staged)
            total_ += (bytes + 255) & ~size_t(255); // rt_ray and rt_bake_point are read as 16-byte pieces
        return regions_.size() - 1;
    }
    uint8_t *staged(const Copy &c) const { return staging_.get() + regions_[c.region].offset + c.first; }
    uint8_t *host(const Copy &c) const { return static_cast<uint8_t *>(regions_[c.region].caller) + c.first; }

    hipStream_t stream_;
    DevBuf<uint8_t> &staging_;
    bool device_;
    size_t total_ = 0;
    std::vector<Region> regions_;
    std::vector<Copy> ups_, downs_;
};

} // namespace rt
