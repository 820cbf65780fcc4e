// rt_env_host.cpp — rt_set_environment (include/rt_abi.h): a float radiance map in place of the scene's background lookup, and optionally the
// tables of its piecewise-constant distribution. The host checks the arguments and computes the H band factors (the solid angle of a cell
// of row i, in double); texels, weights, scans and normalisation are rt_env.hip's. The new buffers are made beside the live ones, then
// swapped in and the old ones freed, so a refusal or a failure leaves the scene unchanged.
#include <cmath>
#include <vector>

#include "rt_env.h"
#include "rt_scene_impl.h"

namespace {

void drop_environment(rt_scene *s) {
    s->env_owned.reset();
    s->dev.env = DevEnv{};
}

} // namespace

extern "C" int rt_set_environment(rt_scene *s, const rt_environment *env) {
    if (!s)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_set_environment: null scene");
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_set_environment: a multi-GPU scene keeps the background it was created with");
    if (s->live_accums)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_set_environment: the scene has " + std::to_string(s->live_accums) +
                                                " live accumulator(s), whose sums are of the old environment: destroy them first");
    HIP_TRY(hipSetDevice(s->device));
    if (!env) { // back to what rt_create made of desc.bg_texture: DevScene::bg_tex was never touched
        HIP_TRY(hipStreamSynchronize(s->stream));
        drop_environment(s);
        return RT_OK;
    }
    if (env->width < 1u || env->width > 8192u || env->height < 1u || env->height > 4096u)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_set_environment: the map must be 1..8192 x 1..4096 texels");
    if (!env->rgb)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_set_environment: null texels");
    if (env->flags & ~(uint32_t)RT_ENV_IMPORTANCE)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_set_environment: unknown flag");
    if (env->reserved)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_set_environment: reserved field is not 0");
    const uint32_t W = env->width, H = env->height;
    const size_t n = (size_t)W * H;
    for (size_t k = 0; k < 3 * n; ++k)
        if (!(std::isfinite(env->rgb[k]) && env->rgb[k] >= 0.0f))
            return rt::fail(RT_ERR_INVALID_ARG, "rt_set_environment: texel " + std::to_string(k / 3) + " is negative or not finite");

    const bool dist = (env->flags & RT_ENV_IMPORTANCE) != 0;
    // the band factors: row i spans polar angles [pi i / H, pi (i + 1) / H] from +y, a cell of it the solid angle (2 pi / W)(cos_i - cos_(i+1))
    std::vector<double> omega(H);
    std::vector<float> band(2 * (size_t)H + 1);
    {
        const double pi = 3.14159265358979323846;
        std::vector<double> edge(H + 1);
        for (uint32_t i = 0; i <= H; ++i)
            edge[i] = i == 0 ? 1.0 : i == H ? -1.0 : std::cos(pi * (double)i / (double)H);
        for (uint32_t i = 0; i <= H; ++i)
            band[i] = (float)edge[i];
        for (uint32_t i = 0; i < H; ++i) {
            omega[i] = (2.0 * pi / (double)W) * (edge[i] - edge[i + 1]);
            band[H + 1 + i] = (float)omega[i];
        }
    }

    // what a build allocates: the texels and the tables are for the scene, `temp` is the build's own; what is not handed to the scene is
    // freed on every return path
    rt::DevArena keep{16}, tables{16}, temp{16};
    DevEnv E{};
    rt::EnvBuild B{};
    E.width = W, E.height = H;
    int rc;
    auto alloc = [](rt::DevArena &a, size_t bytes, auto **out) -> int {
        if (hipError_t e = a.alloc_bytes(out, bytes); e != hipSuccess)
            return rt::hip_fail(e, "rt_set_environment");
        return RT_OK;
    };
    if ((rc = alloc(keep, n * 16, &E.texels)) != RT_OK || (rc = alloc(temp, n * 12, &B.rgb)) != RT_OK)
        return rc;
    if (dist && ((rc = alloc(tables, ((size_t)H + 1) * 4, &E.marg)) != RT_OK || (rc = alloc(tables, (size_t)H * (W + 1) * 4, &E.rows)) != RT_OK ||
                 (rc = alloc(tables, band.size() * 4, &E.band)) != RT_OK || (rc = alloc(temp, (size_t)H * 8, &B.omega)) != RT_OK ||
                 (rc = alloc(temp, n * 8, &B.weights)) != RT_OK || (rc = alloc(temp, (size_t)H * 8, &B.row_total)) != RT_OK ||
                 (rc = alloc(temp, 8, &B.total)) != RT_OK))
        return rc;
    double total = 0.0;
    rc = rt::queue_and_wait(s->stream, [&]() -> int {
        HIP_TRY(hipMemcpyAsync(const_cast<float *>(B.rgb), env->rgb, n * 12, hipMemcpyHostToDevice, s->stream));
        if (dist) {
            HIP_TRY(hipMemcpyAsync(const_cast<double *>(B.omega), omega.data(), (size_t)H * 8, hipMemcpyHostToDevice, s->stream));
            HIP_TRY(hipMemcpyAsync(const_cast<float *>(E.band), band.data(), band.size() * 4, hipMemcpyHostToDevice, s->stream));
        }
        HIP_TRY(rt::launch_env_build(E, B, s->dev.bg, dist, s->stream));
        if (dist)
            HIP_TRY(hipMemcpyAsync(&total, B.total, 8, hipMemcpyDeviceToHost, s->stream));
        return RT_OK;
    });
    if (rc != RT_OK)
        return rc;
    if (dist && !(total > 0.0)) // every weight is zero: no distribution, the flag acts as if it were not set (the tables die with `tables`)
        E.marg = E.rows = E.band = nullptr;
    else
        keep.adopt(tables);
    drop_environment(s); // the stream is idle: nothing reads the old map
    s->env_owned = std::move(keep);
    s->dev.env = E;
    return RT_OK;
}
