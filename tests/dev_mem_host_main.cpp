// The failure paths of csrc/rt_dev_mem.h on the CPU (tests/test_dev_mem_host.py builds and runs this with the address and undefined-behaviour
// sanitizers): rt::DevArena, rt::DevBuf and the two try macros against a stub allocator that counts live allocations, logs every call, can
// fail the k-th hipMalloc with hipErrorOutOfMemory, and aborts on a double free or on a pointer it never handed out. No HIP runtime is linked:
// the entry points the headers call are defined here, and so is rt::fail.
// Also the builders' shared host steps (csrc/rt_build_host.h): rt::ScratchArena, rt::read_back and rt::scan_total in a builder-shaped function
// on a stub stream, where every stubbed call fails in turn: the stream is drained before the first free on every path.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <set>
#include <string>
#include <vector>

#include "rt_build_host.h"

namespace {
std::set<void *> live;
std::vector<size_t> sizes;  // of every successful hipMalloc, in order
std::string calls;          // 'M' a successful hipMalloc, 'x' a failed one, 'F' a hipFree; on the stream: 'S' hipStreamSynchronize, 'C' hipMemcpyAsync,
                            // 'L' a kernel launch (stub_launch below), and 's', 'c', 'l' their failures
long fail_at = -1, n_malloc = 0; // fail the hipMalloc with this index (0-based); -1: none
long fail_call = -1, n_call = 0; // fail the stubbed call (allocation, copy, launch or synchronise; frees cannot fail) with this index; -1: none
int last_code = 0;
std::string last_msg;
int n_checks = 0;

void reset_stub(long k = -1) {
    if (!live.empty()) {
        std::fprintf(stderr, "stub: %zu allocation(s) still live at the start of a scenario\n", live.size());
        std::abort();
    }
    sizes.clear();
    calls.clear();
    fail_at = k;
    n_malloc = 0;
    fail_call = -1;
    n_call = 0;
}
// a call on the stream: logged, and failed if it is its turn
hipError_t stream_call(char ok, char failed) {
    if (n_call++ == fail_call) {
        calls += failed;
        return hipErrorLaunchFailure;
    }
    calls += ok;
    return hipSuccess;
}
// stands in for RT_LAUNCH_CHECKED: the "kernel" runs at once on the host's stand-in for device memory
hipError_t stub_launch(const std::function<void()> &kernel) {
    const hipError_t e = stream_call('L', 'l');
    if (e == hipSuccess)
        kernel();
    return e;
}
} // namespace

extern "C" hipError_t hipStreamSynchronize(hipStream_t) { return stream_call('S', 's'); }
extern "C" hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) {
    const hipError_t e = stream_call('C', 'c');
    if (e == hipSuccess)
        std::memcpy(dst, src, bytes);
    return e;
}
extern "C" hipError_t hipMalloc(void **p, size_t bytes) {
    if (n_malloc++ == fail_at || n_call++ == fail_call) {
        calls += 'x';
        return hipErrorOutOfMemory; // (*p is left alone, as the runtime leaves it)
    }
    *p = bytes ? std::malloc(bytes) : nullptr;
    if (*p)
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
    std::free(p);
    calls += 'F';
    return hipSuccess;
}
extern "C" const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "some other error"; }
int rt::fail(int code, const std::string &msg) {
    last_code = code;
    last_msg = msg;
    return code;
}

#define CHECK(cond)                                                            \
    do {                                                                       \
        ++n_checks;                                                            \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            return 1;                                                          \
        }                                                                      \
    } while (0)

namespace {
struct Big {
    char c[80];
};
constexpr int N_SEQ = 6;
struct Slots {
    float *a = (float *)8;
    Big *b = (Big *)8;
    char *c = (char *)8;
    double *d = (double *)8;
    void *e = (void *)8;
    const float *f = (const float *)8;
    void *at(int k) const {
        const void *all[N_SEQ] = {a, b, c, d, e, f};
        return const_cast<void *>(all[k]);
    }
};
// the shape of the device-side builders: one scratch arena, one arena of outputs, every call through the macro
hipError_t builder(rt::DevArena &tmp, rt::DevArena &outs, Slots &s, const char **err) {
    HIP_TRY_ERR(tmp.alloc(&s.a, 100));
    HIP_TRY_ERR(outs.alloc(&s.b, 3));
    HIP_TRY_ERR(tmp.alloc(&s.c, 0)); // a request for nothing: one element
    HIP_TRY_ERR(outs.alloc_bytes(&s.d, 0)); // ... or the arena's minimum
    HIP_TRY_ERR(tmp.alloc_bytes(&s.e, 40));
    HIP_TRY_ERR(outs.alloc_bytes(&s.f, 12));
    return hipSuccess;
}
// ... on a stream: scratch that drains, an upload, a scan kernel and its total, an output allocated half-way, a second kernel, a read-back.
// On success *total is the scan's total and sum[0..1] the low and high word of it as the second kernel wrote them.
constexpr int N_STREAM_CALLS = 11; // stubbed calls of the success path, up to the return
const char *const STREAM_CALL_TEXT[N_STREAM_CALLS] = {"tmp.alloc(&values", "tmp.alloc(&offsets", "hipMemcpyAsync(values", "stub_launch(scan", "rt::scan_total(",
                                                      "rt::scan_total(", "rt::scan_total(", "outs.alloc(&result", "stub_launch(fill", "rt::read_back(", "rt::read_back("};
hipError_t stream_builder(rt::DevArena &outs, const std::vector<uint32_t> &h_values, uint64_t *total, uint32_t sum[2], const char **err) {
    const hipStream_t stream = nullptr;
    const size_t n = h_values.size();
    rt::ScratchArena tmp{stream};
    uint32_t *values, *offsets, *result;
    HIP_TRY_ERR(tmp.alloc(&values, n));
    HIP_TRY_ERR(tmp.alloc(&offsets, n));
    HIP_TRY_ERR(hipMemcpyAsync(values, h_values.data(), 4 * n, hipMemcpyHostToDevice, stream));
    const auto scan = [&] {
        uint32_t run = 0;
        for (size_t i = 0; i < n; ++i) {
            offsets[i] = run;
            run += values[i]; // 32 bits, as rocPRIM's scan of 32-bit counts: the last OFFSET fits, the total need not
        }
    };
    HIP_TRY_ERR(stub_launch(scan));
    HIP_TRY_ERR(rt::scan_total(values, offsets, n, stream, total));
    HIP_TRY_ERR(outs.alloc(&result, 2)); // after the first launches: a failure here finds kernels possibly in flight
    const uint64_t t = *total;
    const auto fill = [&] { result[0] = (uint32_t)t, result[1] = (uint32_t)(t >> 32); };
    HIP_TRY_ERR(stub_launch(fill));
    HIP_TRY_ERR(rt::read_back(sum, result, 2, stream));
    return hipSuccess;
}
// ... and of the entry points
int entry_point(rt::DevBuf<float> &b, size_t n) {
    HIP_TRY(b.reserve(n));
    return RT_OK;
}
} // namespace

int main() {
    CHECK(rt::hip_code(hipErrorOutOfMemory) == RT_ERR_OOM);
    CHECK(rt::hip_code(hipErrorNoDevice) == RT_ERR_NO_DEVICE);
    CHECK(rt::hip_code(hipErrorInvalidValue) == RT_ERR_HIP);
    CHECK(rt::hip_fail(hipErrorOutOfMemory, "wide pack: somewhere") == RT_ERR_OOM && last_msg == "wide pack: somewhere: out of memory");

    // ---- an arena sequence whose k-th allocation fails, for every k (k == N_SEQ: none does)
    for (long k = 0; k <= N_SEQ; ++k) {
        reset_stub(k);
        {
            rt::DevArena tmp, outs(16);
            Slots s;
            const char *err = "";
            const hipError_t e = builder(tmp, outs, s, &err);
            if (k == N_SEQ) {
                CHECK(e == hipSuccess && live.size() == (size_t)N_SEQ && tmp.size() == 3 && outs.size() == 3);
                CHECK((sizes == std::vector<size_t>{400, 240, 1, 16, 40, 12})); // every size as asked, the two minimums
                for (int j = 0; j < N_SEQ; ++j)
                    CHECK(live.count(s.at(j)) == 1);
            } else {
                CHECK(e == hipErrorOutOfMemory && rt::hip_code(e) == RT_ERR_OOM);
                CHECK(s.at((int)k) == nullptr);           // the failed slot
                CHECK(live.size() == (size_t)k);          // what came before it is still owned ...
                CHECK(tmp.size() + outs.size() == (size_t)k);
                CHECK(std::string(err).find(k % 2 ? "outs.alloc" : "tmp.alloc") == 0); // the macro names the call
                for (int j = (int)k + 1; j < N_SEQ; ++j)
                    CHECK(s.at(j) == (void *)8);          // nothing ran after it
            }
        }
        CHECK(live.empty()); // ... and gone with the arenas
        std::printf("arena sequence, allocation %ld fails: calls %s\n", k, calls.c_str());
    }

    // ---- the builders' steps on a stream: every stubbed call of the sequence fails in turn (k == N_STREAM_CALLS: none does)
    CHECK(rt::scan_total(0u, 0u) == 0ull && rt::scan_total(7u, 5u) == 12ull);
    CHECK(rt::scan_total(0xFFFFFFFFu, 1u) == 0x100000000ull && rt::scan_total(0xFFFFFFFFu, 0xFFFFFFFFu) == 0x1FFFFFFFEull); // carried in 64 bits
    for (long k = 0; k <= N_STREAM_CALLS; ++k) {
        reset_stub();
        fail_call = k < N_STREAM_CALLS ? k : -1;
        hipError_t e;
        const char *err = "";
        uint64_t total = 0;
        uint32_t sum[2] = {0u, 0u};
        {
            rt::DevArena outs(16);
            e = stream_builder(outs, {5u, 0xFFFFFFFAu, 1u}, &total, sum, &err); // offsets 0, 5, 0xFFFFFFFF: last offset + last value = 2^32
            if (k == N_STREAM_CALLS) {
                CHECK(e == hipSuccess && n_call == N_STREAM_CALLS + 1); // (+ 1: the drain)
                CHECK(total == 0x100000000ull && sum[0] == 0u && sum[1] == 1u);
                CHECK(outs.size() == 1 && live.size() == 1); // the scratch is gone, the output is the caller's
            } else {
                CHECK(e == (calls.find('x') != std::string::npos ? hipErrorOutOfMemory : hipErrorLaunchFailure));
                CHECK(std::string(err).find(STREAM_CALL_TEXT[k]) == 0); // the failing call's own text
                CHECK(live.size() == outs.size());
            }
        }
        CHECK(live.empty()); // every allocation freed exactly once (the stub aborts on a second free), the outputs with their arena
        // the stream is drained after the last launch, copy or failure on it, and before the first free; nothing but frees follows
        const size_t first_free = calls.find('F'), last_work = calls.find_last_of("CcLl"), drain = calls.rfind('S');
        CHECK(drain != std::string::npos && (last_work == std::string::npos || drain > last_work));
        CHECK(first_free == std::string::npos ? drain == calls.size() - 1 : first_free == drain + 1);
        CHECK(calls.find_first_not_of('F', drain + 1) == std::string::npos);
        std::printf("stream sequence, call %ld fails: calls %s\n", k, calls.c_str());
    }

    // ---- a default arena's alloc_bytes of nothing: no allocation, a null pointer, nothing owned
    reset_stub();
    {
        rt::DevArena a;
        void *p = (void *)8;
        CHECK(a.alloc_bytes(&p, 0) == hipSuccess && p == nullptr && a.empty() && live.empty());
    }

    // ---- one allocation taken out: still live after the arena, freed exactly once by the taker
    reset_stub();
    {
        void *taken = nullptr;
        {
            rt::DevArena a(16);
            int *x, *y, *z;
            CHECK(a.alloc(&x, 4) == hipSuccess && a.alloc(&y, 4) == hipSuccess && a.alloc(&z, 4) == hipSuccess);
            taken = a.release(y);
            CHECK(taken == y && a.size() == 2);
            CHECK(a.release(y) == y && a.size() == 2);                          // not the arena's any more: nothing happens
            CHECK(a.release((int *)nullptr) == nullptr && a.size() == 2);
        }
        CHECK(live.size() == 1 && live.count(taken) == 1 && calls == "MMMFF");
        rt::DevArena taker;
        taker.adopt(taken);
        taker.adopt((const void *)nullptr);
        CHECK(taker.size() == 1);
        taker.reset();
        CHECK(live.empty() && calls == "MMMFFF");
        taker.reset(); // nothing left to free (the stub aborts on a second free)
        CHECK(calls == "MMMFFF");
    }

    // ---- hand-over of the whole list: the source is empty, the target frees each pointer once (the stub aborts otherwise)
    reset_stub();
    {
        rt::DevArena target;
        char *t0;
        CHECK(target.alloc(&t0, 7) == hipSuccess);
        {
            rt::DevArena source(16);
            char *p, *q;
            CHECK(source.alloc(&p, 1) == hipSuccess && source.alloc(&q, 2) == hipSuccess);
            target.adopt(source);
            CHECK(source.empty() && target.size() == 3);
        }
        CHECK(live.size() == 3 && calls == "MMM"); // the source died empty
        // move assignment (the light swap of a refit, install_geometry): the old list is freed, the new one taken
        rt::DevArena next;
        char *n0;
        CHECK(next.alloc(&n0, 5) == hipSuccess);
        target = std::move(next);
        CHECK(next.empty() && target.size() == 1 && live.size() == 1 && live.count(n0) == 1 && calls == "MMMMFFF");
        // move construction
        rt::DevArena moved(std::move(target));
        CHECK(target.empty() && moved.size() == 1 && live.size() == 1);
        target.reset();
        next.reset(); // moved-from arenas own nothing
        CHECK(live.size() == 1);
    }
    CHECK(live.empty() && calls == "MMMMFFFF");

    // ---- DevBuf::reserve
    reset_stub();
    {
        rt::DevBuf<float> b;
        CHECK(b.get() == nullptr && b.capacity() == 0);
        CHECK(b.reserve(0) == hipSuccess && b.get() == nullptr && calls.empty()); // nothing asked, nothing allocated
        CHECK(b.reserve(10) == hipSuccess && b.get() != nullptr && b.capacity() == 10 && sizes.back() == 40 && calls == "M");
        float *first = b.get();
        CHECK(b.reserve(10) == hipSuccess && b.reserve(3) == hipSuccess && b.get() == first && b.capacity() == 10 && calls == "M"); // it suffices
        CHECK(b.reserve(11) == hipSuccess && b.capacity() == 11 && sizes.back() == 44 && calls == "MFM"); // the old block goes first
        fail_at = n_malloc; // the next growth fails
        CHECK(b.reserve(100) == hipErrorOutOfMemory && b.get() == nullptr && b.capacity() == 0 && calls == "MFMFx" && live.empty());
        CHECK(b.reserve(100) == hipSuccess && b.capacity() == 100 && calls == "MFMFxM"); // and it recovers
        // through the entry points' macro
        fail_at = n_malloc;
        CHECK(entry_point(b, 1000) == RT_ERR_OOM && last_code == RT_ERR_OOM && last_msg == "b.reserve(n): out of memory" && b.capacity() == 0);
        CHECK(entry_point(b, 8) == RT_OK && b.capacity() == 8);
        // moves: the moved-from buffer owns nothing
        rt::DevBuf<float> c(std::move(b));
        CHECK(b.get() == nullptr && b.capacity() == 0 && c.capacity() == 8 && live.size() == 1);
        rt::DevBuf<float> d;
        CHECK(d.reserve(2) == hipSuccess && live.size() == 2);
        d = std::move(c); // frees d's own block
        CHECK(c.get() == nullptr && c.capacity() == 0 && d.capacity() == 8 && live.size() == 1);
        b.reset();
        c.reset();
        CHECK(live.size() == 1);
        d.reset();
        CHECK(live.empty() && d.get() == nullptr && d.capacity() == 0);
        d.reset(); // idempotent
        CHECK(live.empty());
    }
    CHECK(live.empty());
    std::printf("dev_mem ok: %d checks\n", n_checks);
    return 0;
}
