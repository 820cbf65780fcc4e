// rt_dev_stack.h — the two per-lane traversal stacks: StackMemT (LDS columns + per-lane scratch; megakernel, probes, wf_shade's light walk) and
// RingStackT (LDS ring + global overflow workspace; the wavefront closest-hit kernels).
#pragma once
#include <type_traits>

#include "rt_dev_math.h"

namespace {

// ---------------------------------------------------------------------------------------------- traversal stack
// Deferred far siblings: {child ref, far entry distance, enclosing subtree's local best}. The first LDS_DEPTH
// positions live in LDS, one column per thread (bank = thread % 32: conflict free whatever the lanes' depths);
// deeper positions fall back to per-lane scratch. sp counts only ancestors whose BOTH children were hit, so the LDS
// part serves almost every access (DESIGN.md "traversal stack").
#ifndef RT_LDS_DEPTH
#define RT_LDS_DEPTH 12
#endif
constexpr int LDS_DEPTH = RT_LDS_DEPTH;
template <int LDS_DEPTH> struct StackMemT {
    uint32_t *lds; // [3][LDS_DEPTH][256] dwords, this thread's column starts at lds + threadIdx.x
    // The struct holds POINTERS only (registers after scalar replacement): with the arrays as members the whole object,
    // `lds` included, lived in scratch and every LDS access became a generic flat_load/flat_store behind a scratch load
    // of the pointer. RT_DECLARE_STACK sets the pointers up from a __shared__ array and per-lane overflow arrays.
    uint32_t *ov_ref; // [RT_MAX_STACK - LDS_DEPTH], per-lane scratch
    float *ov_d;
    float *ov_loc;
    DEV void push(int sp, uint32_t ref, float d, float loc) {
        if (sp < LDS_DEPTH) {
            lds[(0 * LDS_DEPTH + sp) * 256] = ref;
            lds[(1 * LDS_DEPTH + sp) * 256] = __float_as_uint(d);
            lds[(2 * LDS_DEPTH + sp) * 256] = __float_as_uint(loc);
        } else {
            ov_ref[sp - LDS_DEPTH] = ref;
            ov_d[sp - LDS_DEPTH] = d;
            ov_loc[sp - LDS_DEPTH] = loc;
        }
    }
    DEV void pop(int sp, uint32_t &ref, float &d, float &loc) {
        // The LDS read is unconditional (clamped slot) and the rare deep entry overrides it: selecting between an LDS and
        // a scratch POINTER would turn both into one generic flat_load.
        const int slot = sp < LDS_DEPTH ? sp : LDS_DEPTH - 1;
        ref = lds[(0 * LDS_DEPTH + slot) * 256];
        d = __uint_as_float(lds[(1 * LDS_DEPTH + slot) * 256]);
        loc = __uint_as_float(lds[(2 * LDS_DEPTH + slot) * 256]);
        if (sp >= LDS_DEPTH) {
            ref = ov_ref[sp - LDS_DEPTH];
            d = ov_d[sp - LDS_DEPTH];
            loc = ov_loc[sp - LDS_DEPTH];
        }
    }
    // pop() inside straight-line wave code: every lane reads some valid LDS slot (sp may be negative or stale on lanes
    // that do not `want` the frame), only wanting lanes look at the overflow part
    DEV void pop_masked(int sp, bool want, uint32_t &ref, float &d, float &loc) {
        const uint32_t slot = (uint32_t)sp < (uint32_t)LDS_DEPTH ? (uint32_t)sp : (uint32_t)(LDS_DEPTH - 1);
        ref = lds[(0 * LDS_DEPTH + slot) * 256];
        d = __uint_as_float(lds[(1 * LDS_DEPTH + slot) * 256]);
        loc = __uint_as_float(lds[(2 * LDS_DEPTH + slot) * 256]);
        // keep the LDS reads where they are: sunk into the branch below they would merge with the scratch loads into
        // generic flat_loads of a selected pointer
        asm volatile("" : "+v"(ref), "+v"(d), "+v"(loc));
        if (want && sp >= LDS_DEPTH) {
            ref = ov_ref[sp - LDS_DEPTH];
            d = ov_d[sp - LDS_DEPTH];
            loc = ov_loc[sp - LDS_DEPTH];
        }
    }
    // light-pdf traversal only needs child refs (bvh.h:237-260 has no ordering / pruning)
    DEV void push_ref(int sp, uint32_t ref) {
        if (sp < LDS_DEPTH)
            lds[(0 * LDS_DEPTH + sp) * 256] = ref;
        else
            ov_ref[sp - LDS_DEPTH] = ref;
    }
    DEV uint32_t pop_ref(int sp) {
        uint32_t ref = lds[(0 * LDS_DEPTH + (sp < LDS_DEPTH ? sp : LDS_DEPTH - 1)) * 256];
        if (sp >= LDS_DEPTH)
            ref = ov_ref[sp - LDS_DEPTH];
        return ref;
    }
};
// The same stack for wf_extend, where deep traversals are the norm (S-10M: a tree ~24 levels deep keeps 8-12 deferred
// siblings pending): the LDS part is a RING that always holds the NEWEST frames. Memory position p (0 = oldest) lives in
// LDS slot p % LDS_DEPTH while p >= base, and in scratch once it has been evicted (p < base). A push into a full ring evicts
// the OLDEST LDS frame to scratch; a pop that finds the ring empty takes one frame back from scratch. Scratch is touched only
// when the depth wanders further than LDS_DEPTH from where it was — with StackMemT's fixed split (positions >= LDS_DEPTH
// always in scratch) every push and pop beyond depth 7 went to scratch: 1.2 scratch pushes per cast on S-sponza (0.65 with
// the ring), 9x HBM write amplification of the kernel's real output, the hit records (profiles/r02_write_amp.txt).
template <int LDS_DEPTH, int WORDS = 3> struct RingStackT {
    // WORDS = 3: the reference traversal's frame {ref, d_far, saved local best}; WORDS = 2: the global-best traversal's {ref, d_far}
    static_assert(WORDS == 2 || WORDS == 3, "a frame is {ref, d_far} or {ref, d_far, saved local best}");
    using Rec = std::conditional_t<WORDS == 3, uint4, uint2>;
    uint32_t *lds; // [WORDS][LDS_DEPTH][256] dwords, this thread's column starts at lds + threadIdx.x
    // Evicted frames go to a global workspace, one record {ref, d_far[, saved local best, -]} per (position, thread),
    // laid out [position][thread of the grid]: an eviction or a refill is ONE 16-byte (8-byte) access (the three per-lane scratch
    // arrays this replaces cost three 4-byte accesses in three different 256-byte rows, i.e. three 32-byte sector writes
    // once the lines left L2), and neighbouring lanes' records of one position share lines.
    Rec *ov;        // this thread's record of position 0
    uint32_t stride; // records per position = threads of the grid
    int base;       // positions [base, newest] are in LDS
    DEV static uint32_t slot_of(uint32_t pos) { // pos % LDS_DEPTH for pos < 64
        if constexpr (LDS_DEPTH == 8)
            return pos & 7u;
        else if constexpr (LDS_DEPTH == 4)
            return pos & 3u;
        else if constexpr (LDS_DEPTH == 16)
            return pos & 15u;
        else {
            // pos / LDS_DEPTH by a full-rate 24-bit multiply (a 32-bit v_mul_lo_u32, which the compiler picks for a plain
            // `*` here, issues at quarter rate), then pos - LDS_DEPTH * q with shifts and adds
            uint32_t q;
            asm("v_mul_u32_u24 %0, %1, %2" : "=v"(q) : "v"(pos), "v"((uint32_t)((65536 + LDS_DEPTH - 1) / LDS_DEPTH)));
            q >>= 16;
            static_assert(LDS_DEPTH == 6 || LDS_DEPTH == 5 || LDS_DEPTH == 12 || LDS_DEPTH == 3 || LDS_DEPTH == 9 || LDS_DEPTH == 10 || LDS_DEPTH == 7, "add the shift/add form of LDS_DEPTH * q");
            const uint32_t m = LDS_DEPTH == 6    ? (q << 2) + (q << 1)
                               : LDS_DEPTH == 5  ? (q << 2) + q
                               : LDS_DEPTH == 12 ? (q << 3) + (q << 2)
                               : LDS_DEPTH == 9  ? (q << 3) + q
                               : LDS_DEPTH == 10 ? (q << 3) + (q << 1)
                               : LDS_DEPTH == 7  ? (q << 3) - q
                                                 : (q << 1) + q;
            return pos - m;
        }
    }
    DEV void reset() { base = 0; }
    DEV void push(int pos, uint32_t ref, float d, float loc = 0.0f) {
        const uint32_t slot = slot_of((uint32_t)pos);
        if (pos - base == LDS_DEPTH) { // ring full: the slot about to be overwritten holds position `base`, the oldest
            if constexpr (WORDS == 3)
                ov[(size_t)base * stride] = make_uint4(lds[(0 * LDS_DEPTH + slot) * 256], lds[(1 * LDS_DEPTH + slot) * 256], lds[(2 * LDS_DEPTH + slot) * 256], 0u);
            else
                ov[(size_t)base * stride] = make_uint2(lds[(0 * LDS_DEPTH + slot) * 256], lds[(1 * LDS_DEPTH + slot) * 256]);
            ++base;
        }
        lds[(0 * LDS_DEPTH + slot) * 256] = ref;
        lds[(1 * LDS_DEPTH + slot) * 256] = __float_as_uint(d);
        if constexpr (WORDS == 3)
            lds[(2 * LDS_DEPTH + slot) * 256] = __float_as_uint(loc);
    }
    DEV void pop(int pos, uint32_t &ref, float &d, float &loc) {
        const uint32_t slot = slot_of((uint32_t)pos);
        ref = lds[(0 * LDS_DEPTH + slot) * 256];
        d = __uint_as_float(lds[(1 * LDS_DEPTH + slot) * 256]);
        if constexpr (WORDS == 3)
            loc = __uint_as_float(lds[(2 * LDS_DEPTH + slot) * 256]);
        if (pos < base) { // the ring is empty: take the frame back from the workspace
            const Rec v = ov[(size_t)pos * stride];
            ref = v.x;
            d = __uint_as_float(v.y);
            if constexpr (WORDS == 3)
                loc = __uint_as_float(v.z);
            base = pos;
        }
    }
    // pop() inside straight-line wave code: every lane reads some valid LDS slot (pos may be negative or stale on lanes
    // that do not `want` the frame), only wanting lanes look at the workspace
    DEV void pop_masked(int pos, bool want, uint32_t &ref, float &d, float &loc) {
        const uint32_t p = (uint32_t)pos < (uint32_t)RT_MAX_STACK ? (uint32_t)pos : 0u;
        const uint32_t slot = slot_of(p);
        ref = lds[(0 * LDS_DEPTH + slot) * 256];
        d = __uint_as_float(lds[(1 * LDS_DEPTH + slot) * 256]);
        if constexpr (WORDS == 3)
            loc = __uint_as_float(lds[(2 * LDS_DEPTH + slot) * 256]);
        // keep the LDS reads where they are: sunk into the branch below they would merge with the global loads into
        // generic flat_loads of a selected pointer
        if constexpr (WORDS == 3)
            asm volatile("" : "+v"(ref), "+v"(d), "+v"(loc));
        else
            asm volatile("" : "+v"(ref), "+v"(d));
        if (want && pos < base) {
            const Rec v = ov[(size_t)pos * stride];
            ref = v.x;
            d = __uint_as_float(v.y);
            if constexpr (WORDS == 3)
                loc = __uint_as_float(v.z);
            base = pos;
        }
    }
};
#define RT_DECLARE_RING_STACK_W(NAME, DEPTH, WORDS, SHARED_ARRAY, OVERFLOW, STRIDE)                                                    \
    RingStackT<(DEPTH), (WORDS)> NAME;                                                                                            \
    NAME.lds = (SHARED_ARRAY) + threadIdx.x;                                                                                      \
    NAME.ov = reinterpret_cast<RingStackT<(DEPTH), (WORDS)>::Rec *>(OVERFLOW) + ((size_t)blockIdx.x * blockDim.x + threadIdx.x); \
    NAME.stride = (STRIDE);                                                                                                       \
    NAME.base = 0
#define RT_DECLARE_RING_STACK(NAME, DEPTH, SHARED_ARRAY, OVERFLOW, STRIDE) RT_DECLARE_RING_STACK_W(NAME, DEPTH, 3, SHARED_ARRAY, OVERFLOW, STRIDE)

#define STACK_LDS_DWORDS(depth, words) ((words) * (depth) * 256) /* one column of `depth` frames of `words` dwords per thread of a 256-thread block */
#define RT_DECLARE_STACK(NAME, DEPTH, SHARED_ARRAY)          \
    uint32_t NAME##_ov_ref[RT_MAX_STACK - (DEPTH)];         \
    float NAME##_ov_d[RT_MAX_STACK - (DEPTH)];              \
    float NAME##_ov_loc[RT_MAX_STACK - (DEPTH)];            \
    StackMemT<(DEPTH)> NAME;                                \
    NAME.lds = (SHARED_ARRAY) + threadIdx.x;                \
    NAME.ov_ref = NAME##_ov_ref;                            \
    NAME.ov_d = NAME##_ov_d;                                \
    NAME.ov_loc = NAME##_ov_loc

} // namespace
