// rt_update_dev.h — what rt_update_geometry_device learns about arrays that are in HBM already (rt_update_dev.hip); internal.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "rt_bvh_device.h"
#include "rt_device_types.h"

namespace rt {

// Everything rt_update_geometry's host loops find out about the arrays (check_update in rt_update.cpp, prepare_geometry's light loop in
// rt_scene.cpp), found by one streaming pass on the device instead.
struct UpdateScan {
    bool bad_material = false;            // some material id >= the material count
    uint32_t first_non_finite = RT_NONE;  // the lowest triangle with a NaN or an infinity among its nine floats (what the host loop names)
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}; // bounds of all vertices: k_bounds' words, decoded
    std::vector<uint32_t> light_prims;    // the emissive triangles in ascending order ...
    std::vector<float> light_pos;         // ... and their nine position floats each, in that order
};

// Scans `in` on `stream` (blocking; writes nothing but its own scratch, which it frees): the two data-dependent refusals, the bounds, and —
// with `want_lights`, and only when neither refusal fired — the compacted emissive triangles. `emissive`: one byte per material.
// Neither result depends on how the blocks are scheduled: the checks reduce with integer min / or, the compaction scatters to offsets
// from an exclusive scan of per-block counts.
hipError_t scan_update_device(const DeviceArrays &in, const std::vector<uint8_t> &emissive, bool want_lights, hipStream_t stream, UpdateScan *out, const char **err);

} // namespace rt
