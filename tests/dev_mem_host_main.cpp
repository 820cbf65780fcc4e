// The failure paths of csrc/rt_dev_mem.h on the CPU (tests/test_dev_mem_host.py builds and runs this with the address and undefined-behaviour
// sanitizers): rt::DevArena, rt::DevBuf and the two try macros against a stub allocator that counts live allocations, logs every call, can
// fail the k-th hipMalloc with hipErrorOutOfMemory, and aborts on a double free or on a pointer it never handed out. No HIP runtime is linked:
// the three entry points the header calls are defined here, and so is rt::fail.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "rt_dev_mem.h"

namespace {
std::set<void *> live;
std::vector<size_t> sizes;  // of every successful hipMalloc, in order
std::string calls;          // 'M' a successful hipMalloc, 'x' a failed one, 'F' a hipFree
long fail_at = -1, n_malloc = 0; // fail the hipMalloc with this index (0-based); -1: none
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
}
} // namespace

extern "C" hipError_t hipMalloc(void **p, size_t bytes) {
    if (n_malloc++ == fail_at) {
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
