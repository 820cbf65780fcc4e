// csrc/rt_wf_policy.h on the CPU (tests/test_wf_policy_host.py builds and runs this with the address and undefined-behaviour sanitizers): the
// decisions launch_wavefront_pass takes from it, walked for every ray depth, with and without the size read-back, over every non-increasing
// sequence of queue sizes drawn from SIZES, and the grid helpers against the expressions they replaced.
//
// A pass is simulated as the host sees it: queue b (the rays entering bounce b) has q[b] rays, q[0] = the pass's paths; bounce b records
// q[b + 1] for bounce b + 2 where the policy says so. What a bounce decides, and what is asserted about it, depends on the sequence only
// through (b, q[b - 2], q[b - 1], q[b]) (check_bounce takes nothing else), so the walk visits every such state once and counts the sequences
// that pass through it: the count must come out as the number of all sequences, C(depth + 9, 9) per depth. For depths up to BRUTE_DEPTH
// every sequence is also written out and walked on its own, and must meet the same number of bounces.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_device_types.h" // RT_MAX_RAY_DEPTH
#include "rt_wf_policy.h"

namespace {
using rt::WfPassPolicy;

constexpr uint32_t SIZES[] = {0u, 1u, 63u, 64u, 65u, 4095u, 4096u, 4097u, 8192u, 1u << 20};
constexpr int N_SIZES = 10, BRUTE_DEPTH = 6;
long n_checks = 0;

#define CHECK(cond)                                                                \
    do {                                                                           \
        ++n_checks;                                                                \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

// Bounce b of a pass of P whose queues b - 2, b - 1, b hold q2 >= q1 >= q0 rays (where they exist). Returns false where the pass ends here.
bool check_bounce(const WfPassPolicy &P, uint32_t b, uint32_t q2, uint32_t q1, uint32_t q0) {
    // the words the host has by now: word k = q[k], recorded by bounce k - 1 for bounce k + 1
    uint32_t words[RT_MAX_RAY_DEPTH + 1];
    std::memset(words, 0xEE, sizeof(words)); // a word nobody recorded must not be read as a size
    if (b >= 2 && P.records_size(b - 2))
        words[b - 1] = q1;
    if (b >= 3 && P.records_size(b - 3))
        words[b - 2] = q2;
    if (P.waits_for_size(b))
        CHECK(b >= 2 && P.records_size(b - 2)); // the word waited for was sent
    const uint32_t bound = P.bound(b, words);
    CHECK(bound >= q0 && bound <= P.paths); // an upper bound of the queue, never above the pass
    CHECK(bound == (P.sizes_read_back && b >= 2 ? q1 : P.paths)); // the rule: the path count at bounces 0 and 1, then the size of queue b - 1
    if (P.waits_for_size(b) && q1 == 0u)
        CHECK(P.ends_pass(b, bound)); // (c) a bound of 0 ends the pass: this bounce and everything behind it launch nothing
    if (P.ends_pass(b, bound)) {
        CHECK(bound == 0u && q0 == 0u);
        return false;
    }
    const bool sorted = P.sorted(b, bound), emits = P.emits_keys(b, bound);
    if (sorted) {
        CHECK(b >= 1);
        const uint32_t bound_before = P.bound(b - 1, words); // what bounce b - 1 decided on (its word is still there)
        CHECK(P.emits_keys(b - 1, bound_before)); // (a) sorted only if the bounce before emitted keys
        CHECK(WfPassPolicy::pad_span(bound_before) >= WfPassPolicy::sort_span(bound)); // (b) the pad fill covers what the sort reads ...
        CHECK(WfPassPolicy::sort_span(bound) >= rt::wf_key_span(q1)); // ... and the sort every position the producer's q1 rays could fill
    }
    if (emits)
        CHECK(b + 1 < P.ray_depth && rt::wf_key_span(q0) <= WfPassPolicy::pad_span(bound)); // somebody may sort them; the regions end inside the fill
    if (!P.sizes_read_back) // (d)
        CHECK(!sorted && !emits && !P.waits_for_size(b) && !P.records_size(b));
    for (size_t span : {WfPassPolicy::sort_span(bound), WfPassPolicy::pad_span(bound)}) // (e)
        CHECK(span % 64u == 0u && span <= (size_t)P.paths + 63u && span >= bound);
    CHECK(sorted == (P.sizes_read_back && b >= 1 && bound >= 4096u)); // the rule itself, spelled out once more: the threshold is 4096 rays
    CHECK(emits == (P.sizes_read_back && b + 1 < P.ray_depth && bound >= 4096u));
    return true;
}

// sequences q[b..depth) below a state, each bounce checked once per state: memo[b][i2][i1][i0] (indices into SIZES; i2 >= i1 >= i0)
struct Walk {
    WfPassPolicy P;
    std::vector<long long> memo, memo_bounces; // sequences below the state, and the bounces that run in them
    size_t at(uint32_t b, int i2, int i1, int i0) const { return ((size_t(b) * N_SIZES + i2) * N_SIZES + i1) * N_SIZES + i0; }
    // returns the number of sequences; adds their bounces to `ran`
    long long from(uint32_t b, int i2, int i1, int i0, long long &ran) {
        const size_t k = at(b, i2, i1, i0);
        if (memo[k] < 0) {
            long long n = 0, r = 0;
            if (!check_bounce(P, b, SIZES[i2], SIZES[i1], SIZES[i0])) {
                n = 1; // q[b - 1] = 0: one way to go on (all zeros), and nothing of it runs
            } else if (b + 1 == P.ray_depth) {
                n = 1, r = 1;
            } else {
                for (int next = 0; next <= i0; ++next) {
                    long long sub = 0;
                    const long long m = from(b + 1, i1, i0, next, sub);
                    n += m, r += sub + m; // this bounce ran in each of them
                }
            }
            memo[k] = n, memo_bounces[k] = r;
        }
        ran += memo_bounces[k];
        return memo[k];
    }
};

long long binomial(int n, int k) {
    long long r = 1;
    for (int i = 1; i <= k; ++i)
        r = r * (n - k + i) / i;
    return r;
}

void brute(const WfPassPolicy &P, std::vector<int> &q, long long &n, long long &ran) {
    if (q.size() == P.ray_depth) {
        ++n;
        for (uint32_t b = 0; b < P.ray_depth; ++b, ++ran)
            if (!check_bounce(P, b, SIZES[q[b >= 2 ? b - 2 : 0]], SIZES[q[b >= 1 ? b - 1 : 0]], SIZES[q[b]]))
                break;
        return;
    }
    for (int next = 0; next <= q.back(); ++next) {
        q.push_back(next);
        brute(P, q, n, ran);
        q.pop_back();
    }
}

void check_policy() {
    long long total = 0;
    for (uint32_t depth = 1; depth <= RT_MAX_RAY_DEPTH; ++depth)
        for (int rb = 0; rb < 2; ++rb) {
            long long n = 0, ran = 0, bn = 0, bran = 0;
            for (int ip = 0; ip < N_SIZES; ++ip) {
                Walk w{WfPassPolicy{SIZES[ip], depth, rb != 0}, {}, {}};
                w.memo.assign(size_t(depth) * N_SIZES * N_SIZES * N_SIZES, -1);
                w.memo_bounces.assign(w.memo.size(), 0);
                n += w.from(0, ip, ip, ip, ran); // q[-2], q[-1]: no such queues, and check_bounce reads q[b - k] only from bounce k on
                if (depth <= (uint32_t)BRUTE_DEPTH) {
                    std::vector<int> q{ip};
                    brute(w.P, q, bn, bran);
                }
            }
            CHECK(n == binomial((int)depth + 9, 9)); // every non-increasing sequence of `depth` sizes
            if (depth <= (uint32_t)BRUTE_DEPTH)
                CHECK(bn == n && bran == ran);
            total += n;
        }
    std::printf("policy: %lld passes walked\n", total);
}

// (f) the grids, against the expressions the three wavefront files used to spell out
void check_grids() {
    for (int num_cus : {1, 80, 256, 304}) {
        const uint32_t cap16 = (uint32_t)num_cus * 16u, cap64 = (uint32_t)num_cus * 64u;
        std::vector<uint64_t> ns{0u, 1u, 255u, 256u, 257u};
        for (uint32_t cap : {cap16, cap64})
            for (uint64_t n : {(uint64_t)cap * 256u - 1u, (uint64_t)cap * 256u, (uint64_t)cap * 256u + 1u})
                ns.push_back(n);
        for (uint64_t n64 : ns) {
            const uint32_t n = (uint32_t)n64;
            { // one thread per item: launch_last_stage
                const int res_blocks = (int)((n + 255u) / 256u);
                CHECK(rt::wf_grid_items(n) == (uint32_t)(res_blocks > 0 ? res_blocks : 1));
            }
            if (n >= 1u) { // ... and launch_wavefront_cast, which had no clamp and is not reached without rays
                const int blocks = (int)((n + 255u) / 256u);
                CHECK(rt::wf_grid_items(n) == (uint32_t)blocks);
            }
            { // grid-stride, 16 per CU: launch_camera_relative, launch_sensor_rays, launch_bake_rays
                const uint32_t blocks = std::min<uint32_t>((n + 255u) / 256u, (uint32_t)num_cus * 16u);
                CHECK(rt::wf_grid_stride(n, num_cus, 16u) == (blocks > 0 ? blocks : 1));
            }
            { // ... the first stage and the folds
                const int gen_blocks = (int)((n + 255u) / 256u < (uint32_t)num_cus * 16u ? (n + 255u) / 256u : (uint32_t)num_cus * 16u);
                CHECK(rt::wf_grid_stride(n, num_cus, 16u) == (uint32_t)(gen_blocks > 0 ? gen_blocks : 1));
            }
            { // ... the identity order
                const uint32_t kb = (n + 255u) / 256u < (uint32_t)num_cus * 16u ? (n + 255u) / 256u : (uint32_t)num_cus * 16u;
                CHECK(rt::wf_grid_stride(n, num_cus, 16u) == (kb > 0 ? kb : 1));
            }
        }
        ns.push_back(0xFFFFFFFFull); // 64-bit input: the bake's fold, 64 per CU
        ns.push_back(9ull * 0xFFFFFFFFull);
        for (uint64_t lanes : ns) {
            const uint32_t bake_blocks = (uint32_t)std::min<uint64_t>((lanes + 255u) / 256u, (uint64_t)num_cus * 64u);
            CHECK(rt::wf_grid_stride(lanes, num_cus, 64u) == (bake_blocks > 0 ? bake_blocks : 1));
        }
    }
}
} // namespace

int main() {
    static_assert(RT_RAY_KEY_PAD == (1u << RT_RAY_KEY_BITS) - 1u, "a pad entry is all ones in the compared bits");
    check_policy();
    check_grids();
    std::printf("wf_policy ok: %ld checks\n", n_checks);
    return 0;
}
