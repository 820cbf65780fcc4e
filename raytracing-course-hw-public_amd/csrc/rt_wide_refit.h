// rt_wide_refit.h — refit of the packed 8-wide tree to new triangle arrays, on the device (rt_wide_refit.hip); internal.
#pragma once
#include <hip/hip_runtime_api.h>

#include "../../include/rt_abi.h"
#include "rt_dev_mem.h"
#include "rt_device_types.h"

namespace rt {

// The raw per-triangle arrays on the device (as rt_scene_desc / rt_geometry_update name them) and the bounds of all their vertices.
struct RefitInput {
    DevArena owned; // refit_upload's allocations; empty where the arrays are the caller's (rt_update_geometry_device): then nothing is freed
    float *pos = nullptr, *nrm = nullptr, *uv = nullptr, *tan = nullptr;
    uint32_t *mat = nullptr;
    uint32_t *bounds = nullptr; // k_bounds' words
    uint32_t n = 0;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
};
// Step 1, which writes nothing a render kernel reads: uploads the five arrays of `upd` and reduces the vertex bounds (blocking). The caller
// derives the new WideGrid from lo / hi and may still refuse the update. The arrays live as long as `in` (in->owned).
hipError_t refit_upload(const rt_geometry_update *upd, hipStream_t stream, RefitInput *in, const char **err);

// Step 2: rewrites DevTri[k] / DevAttr[k] of every record for the triangle it names (DevTri::prim), then every node of the blob bottom-up, level
// by level: exact boxes by min / max, origin / exponents / planes by the builders' rule on `grid` (wide_grid.h), the refreshed triangle
// records copied behind their nodes. The topology words (group bases, slot states, DevTri::pad) are read, never written. Blocking; its
// scratch (6 floats per node and per triangle, two words per node) is freed before it returns. hipErrorOutOfMemory leaves every buffer
// as it was: the scratch is allocated before the first write. `levels_ms` (optional): wall time of the top-down level pass, k_refit_level and
// its one host read per level — the part that depends on the topology alone.
hipError_t refit_wide_device(const RefitInput &in, DevTri *tris, DevAttr *attrs, uint32_t n_tris, uint4_pod *blob, uint32_t n_units, uint32_t n_wide,
                             const WideGrid &grid, hipStream_t stream, const char **err, double *levels_ms = nullptr);

} // namespace rt
