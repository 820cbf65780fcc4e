// rt_dev_queue.h — how the persistent closest-hit kernels take work from the ray queue: tickets, the refill of idle lanes, the packet census.
#pragma once
#include "rt_dev_math.h"

namespace {

// ---- work tickets of the persistent closest-hit kernels. Eight heads: the queue — in ray order, i.e. sorted by origin cell and direction when a
// sort ran — is cut into eight contiguous parts and a block starts on part blockIdx.x % 8. Blocks b and b + 8 are observed to share an XCD
// (MI355X_MICROARCH.md, workgroup dispatch), so the rays one XCD's L2 serves are neighbours in that order; a block whose part has run dry moves on
// to the next one. Placement changes speed only: every position is handed out exactly once. Measured against one head for the whole queue
// (profiles/r03_variants.txt item 16): S-10M production 250.7 -> 256.2 Msamples/s, parity +0.5 %; S-sponza (cache resident) unchanged.
struct TicketState {
    uint32_t part, tried; // wave-uniform
};
DEV TicketState ticket_init() { return TicketState{blockIdx.x & 7u, 0u}; }
// next range [q_lo, q_hi) of at most `chunk` queue positions; false = the whole queue has been handed out
DEV bool ticket_take(uint32_t *counters, uint32_t n_in, uint32_t chunk, TicketState &ts, uint32_t &q_lo, uint32_t &q_hi) {
    const uint32_t n_chunks = (n_in + chunk - 1u) / chunk;
    for (;;) {
        if (ts.tried >= 8u)
            return false;
        const uint32_t c0 = (uint32_t)(((unsigned long long)n_chunks * ts.part) >> 3), c1 = (uint32_t)(((unsigned long long)n_chunks * (ts.part + 1u)) >> 3);
        uint32_t t = 0;
        if ((threadIdx.x & 63u) == 0u)
            t = atomicAdd(counters + WF_CNT_XCD + ts.part * WF_CNT_XCD_STRIDE, 1u);
        t = (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
        if (c0 + t < c1) {
            q_lo = (c0 + t) * chunk;
            q_hi = q_lo + chunk < n_in ? q_lo + chunk : n_in;
            return true;
        }
        ts.part = (ts.part + 1u) & 7u; // this part is used up: help the next one
        ++ts.tried;
    }
}
// The refill of the per-lane persistent kernels (wf_extend, wf_extend_wide). A wave refills its idle lanes once `refill_min` of them have finished
// (a refill stalls the wave on the ray loads) from its private range [q_lo, q_hi) of queue positions; a new range of `chunk` positions is taken
// with ONE atomic when it runs dry (a single ticket word saturates near 90 M atomics/s, so tickets are taken per chunk, not per refill).
// start(jq) begins the traversal of the ray at queue position jq in the calling lane; `exhausted` (wave-uniform): the queue is used up.
// Returns the number of idle lanes it found: once `exhausted` no lane is started any more, so that is the wave's idle count.
template <class START>
DEV int ticket_refill(uint32_t *counters, uint32_t n_in, uint32_t chunk, int refill_min, bool idle, bool &exhausted, uint32_t &q_lo, uint32_t &q_hi, TicketState &tks, START start) {
    const unsigned long long im = __ballot(idle);
    const int n_idle = __popcll(im);
    if (!exhausted && (n_idle >= refill_min || n_idle == (int)__popcll(__ballot(1)))) {
        if (q_lo == q_hi)
            exhausted = !ticket_take(counters, n_in, chunk, tks, q_lo, q_hi);
        const uint32_t rank = lane_rank(im);
        const uint32_t avail = q_hi - q_lo;
        if (idle && rank < avail)
            start(q_lo + rank);
        q_lo += (uint32_t)n_idle < avail ? (uint32_t)n_idle : avail;
    }
    return n_idle;
}
// the packet kernels' census (trips, lanes served; wave-uniform), summed over the launch's waves: what the host keeps or drops a packet kernel on
DEV void census_flush(unsigned long long *census, unsigned long long n_trips, unsigned long long n_lanes) {
    if ((threadIdx.x & 63u) == 0u && census && n_trips != 0ull) {
        atomicAdd(census, n_trips);
        atomicAdd(census + 1, n_lanes);
    }
}

} // namespace
