// The failure paths of csrc/rt_call_io.h on the CPU (tests/test_call_io_host.py builds and runs this with the address and undefined-behaviour
// sanitizers): rt::CallIo and rt::queue_and_wait against a stub runtime whose stream is a list of DEFERRED operations. An asynchronous copy
// or a "kernel" (a host lambda handed to stub_launch) is only recorded; the next hipStreamSynchronize carries the list out in order, so
// anything still on it when an entry point returns is work in flight over memory the caller may free. The k-th runtime call of a scenario
// (allocation, copy, launch or synchronise) can be made to fail. No HIP runtime is linked: what the headers call is defined here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <set>
#include <string>
#include <vector>

#include "rt_call_io.h"

namespace {
std::set<void *> live;
std::vector<size_t> sizes;                // of every successful hipMalloc, in order
std::string calls;                        // 'M' hipMalloc, 'F' hipFree, 'U' copy to the device, 'D' copy to the host, 'K' launch, 'S' synchronise; lower case: it failed
std::vector<std::function<void()>> pending; // the stream
long fail_at = -1, n_calls = 0;           // fail the runtime call with this index (0-based, frees not counted); -1: none
int n_checks = 0;

bool fails() { return n_calls++ == fail_at; }
void reset_stub(long k) {
    sizes.clear();
    calls.clear();
    fail_at = k;
    n_calls = 0;
}
hipError_t stub_launch(std::function<void()> kernel) {
    if (fails()) {
        calls += 'k';
        return hipErrorLaunchFailure;
    }
    calls += 'K';
    pending.push_back(std::move(kernel));
    return hipSuccess;
}
} // namespace

extern "C" hipError_t hipMalloc(void **p, size_t bytes) {
    if (fails()) {
        calls += 'm';
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(bytes);
    live.insert(*p);
    sizes.push_back(bytes);
    calls += 'M';
    return hipSuccess;
}
extern "C" hipError_t hipFree(void *p) {
    if (!p || live.erase(p) != 1) {
        std::fprintf(stderr, "stub: hipFree(%p): null, freed twice or never allocated\n", p);
        std::abort();
    }
    if (!pending.empty()) {
        std::fprintf(stderr, "stub: hipFree(%p) with %zu operation(s) in flight\n", p, pending.size());
        std::abort();
    }
    std::free(p);
    calls += 'F';
    return hipSuccess;
}
extern "C" hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    const bool up = kind == hipMemcpyHostToDevice;
    if (fails()) {
        calls += up ? 'u' : 'd';
        return hipErrorInvalidValue;
    }
    calls += up ? 'U' : 'D';
    pending.push_back([=] { std::memcpy(dst, src, bytes); });
    return hipSuccess;
}
extern "C" hipError_t hipStreamSynchronize(hipStream_t) {
    for (auto &op : pending) // a synchronise that reports a failure has still waited
        op();
    pending.clear();
    const bool f = fails();
    calls += f ? 's' : 'S';
    return f ? hipErrorUnknown : hipSuccess;
}
extern "C" hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    if (hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, nullptr); e != hipSuccess)
        return e;
    return hipStreamSynchronize(nullptr);
}
extern "C" const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "some other error"; }
int rt::fail(int code, const std::string &) { return code; }

#define CHECK(cond)                                                            \
    do {                                                                       \
        ++n_checks;                                                            \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                          \
        }                                                                      \
    } while (0)

namespace {
constexpr size_t GUARD = 32;
constexpr uint8_t SENTINEL = 0xA5;
uint8_t in_byte(int which, size_t j) { return (uint8_t)(17u * which + 31u * j + (j >> 3)); }
uint8_t out_byte(int which, size_t j, const uint8_t *in0, size_t n0, const uint8_t *in1, size_t n1) { return (uint8_t)(in0[j % n0] ^ (in1[(3 * j) % n1] + 7u * which + j)); }

// One call with two inputs and three outputs (the last destination null) on `owner`; the k-th runtime call fails. 0: every check passed.
// `sz`: the five sizes, unequal and no multiple of 16.
int one_call(rt::DevBuf<uint8_t> &owner, bool device, const size_t (&sz)[5], long k, int *rc_out) {
    std::vector<uint8_t> in[2], dst[3]; // the caller's arrays: on the host, or "in HBM" (the stub's device memory is the host's)
    for (int i = 0; i < 2; ++i)
        for (size_t j = 0; j < sz[i]; ++j)
            in[i].push_back(in_byte(i, j));
    for (int o = 0; o < 3; ++o)
        dst[o].assign(sz[2 + o] + GUARD, SENTINEL);
    uint8_t *const want[3] = {dst[0].data(), dst[1].data(), nullptr};
    reset_stub(k);
    int kernel_error = 0;
    {
        rt::CallIo io(nullptr, owner, device);
        const uint8_t *d_in[2] = {(const uint8_t *)8, (const uint8_t *)8};
        uint8_t *d_out[3] = {(uint8_t *)8, (uint8_t *)8, (uint8_t *)8};
        for (int i = 0; i < 2; ++i)
            io.in(&d_in[i], in[i].data(), sz[i]);
        for (int o = 0; o < 3; ++o)
            io.out(&d_out[o], want[o], sz[2 + o]);
        for (int i = 0; i < 5; ++i)
            CHECK((i < 2 ? (const void *)d_in[i] : (const void *)d_out[i - 2]) == nullptr); // nothing is handed out before the reservation
        auto kernel = [&] { // runs at the synchronise, behind the uploads
            for (int i = 0; i < 2; ++i)
                if (std::memcmp(d_in[i], in[i].data(), sz[i]) != 0) // an upload carries the caller's bytes
                    kernel_error = 1;
            for (int o = 0; o < 3; ++o)
                for (size_t j = 0; d_out[o] && j < sz[2 + o]; ++j)
                    d_out[o][j] = out_byte(o, j, d_in[0], sz[0], d_in[1], sz[1]);
        };
        *rc_out = io.run([&]() -> int {
            HIP_TRY(stub_launch(kernel));
            return RT_OK;
        });
        CHECK(pending.empty()); // on every path: nothing in flight at return
        const bool reserved = calls.find('m') == std::string::npos;
        if (device) {
            CHECK(calls.find_first_of("MmUuDd") == std::string::npos && live.empty()); // no allocation, no copy
            CHECK(d_in[0] == in[0].data() && d_in[1] == in[1].data() && d_out[0] == want[0] && d_out[1] == want[1] && d_out[2] == nullptr);
        } else if (reserved) { // regions: inside the block, aligned, disjoint
            const uint8_t *lo = owner.get(), *hi = lo + owner.capacity();
            const uint8_t *r[5] = {d_in[0], d_in[1], d_out[0], d_out[1], d_out[2]};
            for (int a = 0; a < 5; ++a) {
                CHECK(r[a] >= lo && r[a] + sz[a] <= hi && (reinterpret_cast<uintptr_t>(r[a]) & 15u) == 0);
                for (int b = 0; b < a; ++b)
                    CHECK(r[a] + sz[a] <= r[b] || r[b] + sz[b] <= r[a]);
            }
            CHECK(std::count(calls.begin(), calls.end(), 'D') + std::count(calls.begin(), calls.end(), 'd') <= 2); // none for the null destination
        } else {
            CHECK(*rc_out == RT_ERR_OOM && owner.get() == nullptr && owner.capacity() == 0);
        }
    }
    CHECK(kernel_error == 0);
    CHECK((*rc_out == RT_OK) == (k < 0 || k >= n_calls)); // a failed runtime call fails the entry point, and nothing else does
    for (int o = 0; o < 3; ++o) {
        for (size_t j = 0; want[o] && *rc_out == RT_OK && j < sz[2 + o]; ++j)
            CHECK(dst[o][j] == out_byte(o, j, in[0].data(), sz[0], in[1].data(), sz[1])); // bit-equal to what the kernel wrote
        for (size_t j = sz[2 + o]; j < dst[o].size(); ++j)
            CHECK(dst[o][j] == SENTINEL); // beyond the declared size: untouched
    }
    return 0;
}
} // namespace

int main() {
    const size_t small[5] = {37, 1001, 5, 333, 77}, large[5] = {41, 3003, 9, 777, 1234}, tiny[5] = {3, 21, 1, 7, 11};
    for (int device = 0; device < 2; ++device) {
        long n_success = 0;
        for (long k = -1; k == -1 || k < n_success; ++k) { // none fails, then every runtime call of the successful sequence in turn
            int rc = -1;
            {
                rt::DevBuf<uint8_t> owner;
                if (one_call(owner, device != 0, small, k, &rc) != 0)
                    return 1;
                CHECK(device ? live.empty() : live.size() <= 1);
            }
            CHECK(live.empty()); // no allocation outlives the owner
            if (k == -1) {
                CHECK(rc == RT_OK && calls == (device ? "KS" : "MUUKDDSF")); // (the owner has died: its free)
                n_success = n_calls;
            }
            std::printf("%s call, runtime call %ld fails: rc %d calls %s\n", device ? "device" : "host", k, rc, calls.c_str());
        }
    }

    // ---- growth: the same owner over three calls; the old block is freed before the larger one is asked for, a smaller call allocates nothing
    {
        rt::DevBuf<uint8_t> owner;
        int rc = -1;
        std::string all;
        for (const auto *sz : {&small, &large, &tiny}) {
            if (one_call(owner, false, *sz, -1, &rc) != 0)
                return 1;
            CHECK(rc == RT_OK);
            all += calls;
        }
        CHECK(all == "MUUKDDS" "FMUUKDDS" "UUKDDS" && live.size() == 1);
        std::printf("growth: calls %s\n", all.c_str());
    }
    CHECK(live.empty());

    // ---- scratch is staged also on a device call; of a ranged output only the named bytes come back, in a run of their own if need be
    {
        rt::DevBuf<uint8_t> owner;
        reset_stub(-1);
        std::vector<uint8_t> dst(100, SENTINEL), hbm(100, SENTINEL);
        uint8_t *d_a, *d_b, *d_tmp;
        rt::CallIo dev(nullptr, owner, true);
        dev.scratch(&d_tmp, 50);
        dev.out(&d_a, hbm.data(), 100);
        CHECK(dev.run([] { return RT_OK; }) == RT_OK && calls == "MS" && d_a == hbm.data() && d_tmp == owner.get() && owner.capacity() >= 50);
        rt::CallIo host(nullptr, owner, false);
        const size_t h = host.out_ranges(&d_b, dst.data(), 100);
        host.range(h, 10, 5);
        CHECK(host.run([&]() -> int { return stub_launch([&] { std::memset(d_b, 1, 100); }) == hipSuccess ? RT_OK : RT_ERR_HIP; }) == RT_OK);
        host.range(h, 90, 10);
        CHECK(rt::queue_and_wait(nullptr, [&] { return host.download(); }) == RT_OK && pending.empty());
        for (size_t j = 0; j < 100; ++j)
            CHECK(dst[j] == (((j >= 10 && j < 15) || j >= 90) ? 1 : SENTINEL));
    }
    CHECK(live.empty());
    std::printf("call_io ok: %d checks\n", n_checks);
    return 0;
}
