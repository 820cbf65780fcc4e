// rt_shutter.h — the two kernels of a shutter accumulator (rt_shutter.hip; rt_abi.h rt_accum_attach_shutter states the rule); internal.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace rt {

// The three interpolated arrays of a triangle soup (positions, normals, tangents: 9 floats per triangle each), all device memory.
struct ShutterArrays {
    float *a[3] = {nullptr, nullptr, nullptr};
};

// out = the geometry at time t, float by float (the rule's "geometry at t"): one launch over the 3 x 9n floats. `out` may alias neither key.
hipError_t launch_shutter_blend(const ShutterArrays &key0, const ShutterArrays &key1, const ShutterArrays &out, uint32_t n_triangles, float t, hipStream_t stream);

// *d_moving (one device word, zeroed by the launch's stream beforehand) becomes non-zero when some triangle whose material emits
// (`d_emissive`: one byte per material; ids >= n_materials are skipped, the update scan refuses them) has a position float whose two keys
// differ in any bit. Integer OR: no order dependence.
hipError_t launch_shutter_moving_lights(const float *pos0, const float *pos1, const uint32_t *mat, const uint8_t *d_emissive, uint32_t n_materials,
                                        uint32_t n_triangles, uint32_t *d_moving, hipStream_t stream);

} // namespace rt
