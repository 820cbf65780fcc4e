// rt_env_host.cpp — rt_set_environment (include/rt_abi.h): a float radiance map in place of the scene's background lookup, and optionally the
// tables of its piecewise-constant distribution. The host checks the arguments and computes the H band factors (the solid angle of a cell
// of row i, in double); texels, weights, scans and normalisation are rt_env.hip's. The new buffers are made beside the live ones, then
// swapped in and the old ones freed, so a refusal or a failure leaves the scene unchanged.
#include <cmath>
#include <vector>

#include "rt_env.h"
#include "rt_scene_impl.h"

namespace {

struct DevBufs { // everything a build allocates; what is not handed to the scene is freed on every return path
    std::vector<void *> p;
    int alloc(size_t bytes, void **out) {
        *out = nullptr;
        const hipError_t e = hipMalloc(out, bytes ? bytes : 16);
        if (e != hipSuccess)
            return rt::fail(e == hipErrorOutOfMemory ? RT_ERR_OOM : RT_ERR_HIP, std::string("rt_set_environment: ") + hipGetErrorString(e));
        p.push_back(*out);
        return RT_OK;
    }
    ~DevBufs() {
        for (void *q : p)
            (void)hipFree(q);
    }
};

void drop_environment(rt_scene *s) {
    for (void *q : s->env_owned)
        (void)hipFree(q);
    s->env_owned.clear();
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

    DevBufs keep, temp;
    DevEnv E{};
    rt::EnvBuild B{};
    E.width = W, E.height = H;
    int rc;
    if ((rc = keep.alloc(n * 16, (void **)&E.texels)) != RT_OK || (rc = temp.alloc(n * 12, (void **)&B.rgb)) != RT_OK)
        return rc;
    if (dist && ((rc = keep.alloc(((size_t)H + 1) * 4, (void **)&E.marg)) != RT_OK || (rc = keep.alloc((size_t)H * (W + 1) * 4, (void **)&E.rows)) != RT_OK ||
                 (rc = keep.alloc(band.size() * 4, (void **)&E.band)) != RT_OK || (rc = temp.alloc((size_t)H * 8, (void **)&B.omega)) != RT_OK ||
                 (rc = temp.alloc(n * 8, (void **)&B.weights)) != RT_OK || (rc = temp.alloc((size_t)H * 8, (void **)&B.row_total)) != RT_OK ||
                 (rc = temp.alloc(8, (void **)&B.total)) != RT_OK))
        return rc;
    double total = 0.0;
    rc = rt::queue_and_wait(s, [&]() -> int {
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
    if (dist && !(total > 0.0)) // every weight is zero: no distribution, the flag acts as if it were not set (the tables go with `keep`)
        E.marg = E.rows = E.band = nullptr;
    drop_environment(s); // the stream is idle: nothing reads the old map
    for (void *q : keep.p)
        if (q == E.texels || E.marg)
            s->env_owned.push_back(q);
        else
            (void)hipFree(q);
    keep.p.clear();
    s->dev.env = E;
    return RT_OK;
}
