// rt_build_scan.h — rocPRIM's exclusive scan of 32-bit counts as the builders use it (PLOC's compaction, the wide pack's group bases, the
// update scan's light offsets): ask for the size, allocate the scratch, run. Its total is rt::scan_total (rt_build_host.h). Internal; includes
// rocPRIM, so only .hip files include it.
#pragma once
#include <cstring> // rocPRIM's headers call memset without including it

#include <rocprim/rocprim.hpp>

#include "rt_build_host.h"

namespace rt {

struct ExclusiveScan {
    void *tmp = nullptr;
    size_t bytes = 0;
    // scratch for scans of up to `n_max` values, from `arena`
    hipError_t prepare(DevArena &arena, uint32_t *values, uint32_t *offsets, size_t n_max, hipStream_t stream) {
        const hipError_t e = rocprim::exclusive_scan(nullptr, bytes, values, offsets, 0u, n_max, rocprim::plus<uint32_t>(), stream);
        return e != hipSuccess ? e : arena.alloc_bytes(&tmp, bytes ? bytes : 1); // never null: a null scratch is rocPRIM's size query
    }
    // offsets[i] = values[0] + ... + values[i - 1], n <= n_max
    hipError_t run(uint32_t *values, uint32_t *offsets, size_t n, hipStream_t stream) const {
        size_t b = bytes;
        return rocprim::exclusive_scan(tmp, b, values, offsets, 0u, n, rocprim::plus<uint32_t>(), stream);
    }
};

} // namespace rt
