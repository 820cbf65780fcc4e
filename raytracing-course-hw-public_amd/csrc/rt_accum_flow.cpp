// rt_accum_flow.cpp — the motion vectors of an accumulator (rt_abi.h rt_accum_attach_flow: the rule; include/rt_flowspec.h: the rule as code):
// attach, read and resolve of the fourth layer (rt_accum_impl.h; the first three are rt_accum_layers.cpp). The passes that fill it are
// rt_accum_host.cpp's; the kernels are rt_wavefront.hip (wf_flow), rt_wf_stages.h (wf_resolve_flow) and rt_accum.hip (the image). The keys go
// through the one staging path (rt_call_io.h) into the accumulator's arena, and their positions through the update path's check kernel
// (rt_update.cpp refuse_non_finite_positions) before the layer is published.
#include "rt_accum_impl.h"

using rt::AccumNeed;

namespace {
const std::string FN = "rt_accum_attach_flow";
}

extern "C" int rt_accum_attach_flow(rt_accum *acc, const rt_flow_desc *desc) {
    if (!acc || !desc)
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": null argument");
    rt_scene *s = acc->scene;
    for (uint32_t r : desc->reserved)
        if (r != 0)
            return rt::fail(RT_ERR_INVALID_ARG, FN + ": reserved fields must be 0");
    if (rt::other_flags(desc->flags))
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": flags other than RT_FLAG_DEVICE_FB");
    const uint32_t n = desc->n_triangles;
    const bool device = (desc->flags & RT_FLAG_DEVICE_FB) != 0;
    if (n != 0 && n != s->dev.n_triangles)
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": n_triangles is " + std::to_string(n) + ", the scene has " + std::to_string(s->dev.n_triangles) + " (or 0: no triangle moves)");
    if (n)
        for (const float *p : desc->positions) {
            if (!p)
                return rt::fail(RT_ERR_INVALID_ARG, FN + ": null key");
            if (device && ((uintptr_t)p & 3u))
                return rt::fail(RT_ERR_INVALID_ARG, FN + ": misaligned key (device pointers must be 4-byte aligned)");
        }
    if (desc->sensor1) {
        if (desc->sensor1->kind != acc->sensor_desc.kind)
            return rt::fail(RT_ERR_INVALID_ARG, FN + ": sensor1 is of kind " + std::to_string(desc->sensor1->kind) + ", the accumulator's view of kind " + std::to_string(acc->sensor_desc.kind));
        if (int rc = rt::check_sensor(*desc->sensor1, acc->width, acc->height, FN.c_str()); rc != RT_OK)
            return rc;
    }
    if (acc->flow)
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": the accumulator already has flow");
    if (acc->has_samples)
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": the accumulator already holds samples; attach flow before the first render");
    if (acc->shutter)
        return rt::fail(RT_ERR_UNSUPPORTED, FN + ": the accumulator has a shutter (rt_accum_attach_shutter); a slice's geometry is not key 0");
    HIP_TRY(hipSetDevice(s->device));
    const size_t f9 = 36 * (size_t)n, pixels = (size_t)acc->width * acc->height;
    if (n && device)
        for (const float *p : desc->positions)
            if (int rc = rt::check_device_array(s, p, f9, FN); rc != RT_OK)
                return rc;
    WfFlow W{};
    W.n_triangles = n;
    W.pixels = (uint32_t)pixels;
    rt::DevArena arena; // the accumulator's only once nothing can be refused any more
    auto alloc = [&]<class T>(T **p, size_t bytes) -> int {
        if (hipError_t e = arena.alloc_bytes(p, bytes); e != hipSuccess)
            return rt::hip_fail(e, FN);
        return RT_OK;
    };
    float *key[2] = {nullptr, nullptr};
    WfSensor *d_sensor1 = nullptr;
    int rc;
    if ((rc = alloc(&W.flow_sum, 8 * pixels)) != RT_OK || (rc = alloc(&W.valid, 4 * pixels)) != RT_OK || (rc = alloc(&W.near_flow, 8 * pixels)) != RT_OK ||
        (rc = alloc(&W.near_t, 4 * pixels)) != RT_OK)
        return rc;
    if (n && ((rc = alloc(&key[0], f9)) != RT_OK || (rc = alloc(&key[1], f9)) != RT_OK))
        return rc;
    if (desc->sensor1 && (rc = alloc(&d_sensor1, sizeof(WfSensor))) != RT_OK)
        return rc;
    const WfSensor rec1 = desc->sensor1 ? rt::make_sensor(*desc->sensor1, acc->width, acc->height) : WfSensor{};
    // ---- the keys, host or device, to the accumulator's own copies; the sums start from +0.0
    rt::CallIo io(s->stream, s->staging, device);
    const float *src[2];
    for (int k = 0; k < 2; ++k)
        io.in(&src[k], n ? desc->positions[k] : nullptr, f9);
    rc = io.run([&]() -> int {
        for (int k = 0; k < 2 && n; ++k)
            HIP_TRY(hipMemcpyAsync(key[k], src[k], f9, hipMemcpyDeviceToDevice, s->stream));
        HIP_TRY(hipMemsetAsync(W.flow_sum, 0, 8 * pixels, s->stream));
        HIP_TRY(hipMemsetAsync(W.valid, 0, 4 * pixels, s->stream));
        HIP_TRY(hipMemsetAsync(W.near_flow, 0, 8 * pixels, s->stream));
        HIP_TRY(hipMemsetAsync(W.near_t, 0, 4 * pixels, s->stream));
        if (d_sensor1)
            HIP_TRY(hipMemcpyAsync(d_sensor1, &rec1, sizeof(WfSensor), hipMemcpyHostToDevice, s->stream)); // `rec1` outlives the bracket's wait
        return RT_OK;
    });
    if (rc != RT_OK)
        return rc;
    // ---- a non-finite position in either key, by the update path's check kernel over the copies (the lowest triangle is named)
    for (int k = 0; k < 2 && n; ++k)
        if ((rc = rt::refuse_non_finite_positions(s, key[k], n, FN + " (key " + std::to_string(k) + ")")) != RT_OK)
            return rc;
    W.key[0] = key[0], W.key[1] = key[1];
    W.sensor1 = d_sensor1 ? d_sensor1 : acc->d_sensor;
    acc->owned.adopt(arena);
    acc->flow = W;
    return RT_OK;
}

extern "C" int rt_accum_read_flow(rt_accum *acc, float *flow_sum, uint32_t *valid, float *near_flow, float *near_t) {
    if (int rc = rt::accum_entry(acc, "rt_accum_read_flow", AccumNeed::FLOW); rc != RT_OK)
        return rc;
    const WfFlow &F = *acc->flow;
    const size_t n = F.pixels;
    return rt::read_back(acc, {{flow_sum, F.flow_sum, 8 * n}, {valid, F.valid, 4 * n}, {near_flow, F.near_flow, 8 * n}, {near_t, F.near_t, 4 * n}});
}

extern "C" int rt_accum_resolve_flow(rt_accum *acc, uint32_t mode, uint32_t flags, float *flow, float *mask) {
    if (int rc = rt::accum_entry(acc, "rt_accum_resolve_flow", AccumNeed::FLOW); rc != RT_OK)
        return rc;
    if (mode != RT_FLOW_MEAN && mode != RT_FLOW_NEAREST)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_resolve_flow: unknown mode " + std::to_string(mode));
    if (rt::other_flags(flags))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_resolve_flow: flags other than RT_FLAG_DEVICE_FB");
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    rt::CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    float *d_flow, *d_mask; // on a host call both are computed; a null destination is not copied
    io.out(&d_flow, flow, 8 * (size_t)acc->flow->pixels);
    io.out(&d_mask, mask, 4 * (size_t)acc->flow->pixels);
    return io.run([&]() -> int {
        HIP_TRY(rt::launch_accum_flow(acc->R, *acc->flow, mode, d_flow, d_mask, s->stream));
        return RT_OK;
    });
}
