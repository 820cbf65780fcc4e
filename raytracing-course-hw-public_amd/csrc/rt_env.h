// rt_env.h — launchers of rt_env.hip: the build of a float environment's tables on the device and the two distribution probes (internal;
// the rule is include/rt_abi.h rt_set_environment's).
#pragma once
#include <hip/hip_runtime_api.h>

#include "rt_device_types.h"

namespace rt {
// Workspace of one build, all device memory: the caller allocates and frees it (rt_env_host.cpp).
struct EnvBuild {
    const float *rgb;    // [3 * width * height] the caller's texels, as uploaded
    const double *omega; // [height] cell solid angles of row i (the band factors, from the host)
    double *weights;     // [width * height] w_ij
    double *row_total;   // [height]
    double *total;       // [1] sum of every w_ij, for the host to read
};
// texels <- rgb as float4. With `dist`: weights, the per-row CDFs and the marginal into E.rows / E.marg, B.total. Stream-ordered.
hipError_t launch_env_build(const DevEnv &E, const EnvBuild &B, const float *bg, bool dist, hipStream_t stream);
hipError_t launch_env_pdf(const DevEnv &E, const float *dirs, uint32_t n, float *pdf, hipStream_t stream);
hipError_t launch_env_sample(const DevEnv &E, const float *xi4, uint32_t n, float *dirs, hipStream_t stream);
} // namespace rt
