// rt_accum_shutter.cpp — the shutter of an accumulator (rt_abi.h rt_accum_attach_shutter: the rule): attach, the install of a slice, the times.
// The render loop that cuts a call into runs of one slice is rt_accum_host.cpp's; the kernels are rt_shutter.hip; a slice's geometry goes
// through rt_update.cpp's path for device arrays (rt::update_from_device_arrays), which is rt_update_geometry_device behind its checks.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rt_accum_impl.h"
#include "rt_update_dev.h"

namespace {

const std::string FN = "rt_accum_attach_shutter";

// ---- the rule's host half: slice of a sample, time of a slice, sensor at t (IEEE binary32 as written; this file is compiled without contraction)
uint32_t bit_reverse(uint32_t j, uint32_t slices) {
    uint32_t k = 0;
    for (uint32_t bit = 1; bit < slices; bit <<= 1, j >>= 1)
        k = (k << 1) | (j & 1u);
    return k;
}
float slice_time(const rt::Shutter &H, uint32_t k) { return H.open + (H.close - H.open) * (((float)k + 0.5f) / (float)H.slices); }
float blend(float x0, float x1, float t) { return x0 + t * (x1 - x0); }
void blend_axis(const float a0[3], const float a1[3], float t, float out[3]) {
    const float x = blend(a0[0], a1[0], t), y = blend(a0[1], a1[1], t), z = blend(a0[2], a1[2], t);
    const float len = std::sqrt(x * x + y * y + z * z);
    out[0] = x / len, out[1] = y / len, out[2] = z / len;
}
rt_sensor sensor_at(const rt_sensor &s0, const rt_sensor &s1, float t) {
    rt_sensor r = s0; // kind, seed and the reserved words are sensor 0's
    for (int c = 0; c < 3; ++c)
        r.camera.position[c] = blend(s0.camera.position[c], s1.camera.position[c], t);
    r.camera.fov_x = blend(s0.camera.fov_x, s1.camera.fov_x, t);
    r.half_width = blend(s0.half_width, s1.half_width, t);
    r.lens_radius = blend(s0.lens_radius, s1.lens_radius, t);
    r.focus_distance = blend(s0.focus_distance, s1.focus_distance, t);
    blend_axis(s0.camera.right, s1.camera.right, t, r.camera.right);
    blend_axis(s0.camera.up, s1.camera.up, t, r.camera.up);
    blend_axis(s0.camera.forward, s1.camera.forward, t, r.camera.forward);
    return r;
}

rt_geometry_update update_of(const rt::Shutter &H, const rt::ShutterArrays &arrays) {
    rt_geometry_update u{};
    u.n_triangles = H.n;
    u.mode = H.mode;
    u.positions = arrays.a[0], u.normals = arrays.a[1], u.tangents = arrays.a[2];
    u.texcoords = H.uv, u.material_ids = H.mat;
    return u;
}

// what the descriptor alone can be refused for
int check_desc(const rt_shutter_desc *d) {
    for (uint32_t r : d->reserved)
        if (r != 0)
            return rt::fail(RT_ERR_INVALID_ARG, FN + ": reserved fields must be 0");
    if (rt::other_flags(d->flags))
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": flags other than RT_FLAG_DEVICE_FB");
    if (d->mode != RT_UPDATE_REBUILD && d->mode != RT_UPDATE_REFIT)
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": unknown mode");
    if (d->slices == 0 || d->slices > 1024u || (d->slices & (d->slices - 1u)) != 0 || d->block == 0)
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": slices must be a power of two in 1..1024 and block at least 1");
    if (!(0.0f <= d->open && d->open <= d->close && d->close <= 1.0f))
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": open and close must satisfy 0 <= open <= close <= 1");
    if (d->n_triangles) {
        const void *arrays[8] = {d->positions[0], d->positions[1], d->normals[0], d->normals[1], d->tangents[0], d->tangents[1], d->texcoords, d->material_ids};
        for (const void *p : arrays) {
            if (!p)
                return rt::fail(RT_ERR_INVALID_ARG, FN + ": null geometry array");
            if ((d->flags & RT_FLAG_DEVICE_FB) && ((uintptr_t)p & 3u))
                return rt::fail(RT_ERR_INVALID_ARG, FN + ": misaligned geometry array (device pointers must be 4-byte aligned)");
        }
    }
    return RT_OK;
}

} // namespace

uint32_t rt::shutter_slice(const rt::Shutter &H, uint64_t s) { return bit_reverse((uint32_t)((s / H.block) % H.slices), H.slices); }

int rt::shutter_install(rt_accum *a, int k, bool keep_static_lights) {
    rt::Shutter &H = *a->shutter;
    rt_scene *s = a->scene;
    const auto t0 = std::chrono::steady_clock::now();
    const float t = k < 0 ? 0.0f : slice_time(H, (uint32_t)k);
    if (H.n) {
        if (k >= 0)
            HIP_TRY(rt::launch_shutter_blend(H.key[0], H.key[1], H.blend, H.n, t, s->stream));
        const rt_geometry_update u = update_of(H, k < 0 ? H.key[0] : H.blend);
        const bool keep = keep_static_lights && H.static_lights && H.mode == RT_UPDATE_REFIT;
        if (int rc = rt::update_from_device_arrays(s, &u, keep); rc != RT_OK)
            return rc;
        H.light_rebuilds += keep ? 0u : 1u;
    }
    if (H.has_sensor1) {
        a->sensor = rt::make_sensor(k < 0 ? a->sensor_desc : sensor_at(a->sensor_desc, H.sensor1, t), a->width, a->height);
        if (int rc = rt::queue_and_wait(s->stream, [&]() -> int {
                HIP_TRY(hipMemcpyAsync(a->d_sensor, &a->sensor, sizeof(WfSensor), hipMemcpyHostToDevice, s->stream));
                return RT_OK;
            });
            rc != RT_OK)
            return rc;
    }
    if (k >= 0) {
        H.change_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        H.changes += 1;
    }
    return RT_OK;
}

extern "C" int rt_accum_attach_shutter(rt_accum *acc, const rt_shutter_desc *desc) {
    if (!acc || !desc)
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": null argument");
    rt_scene *s = acc->scene;
    if (int rc = check_desc(desc); rc != RT_OK)
        return rc;
    if (acc->shutter)
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": the accumulator already has a shutter");
    if (acc->flow)
        return rt::fail(RT_ERR_UNSUPPORTED, FN + ": the accumulator has flow (rt_accum_attach_flow), whose key 0 is the scene's one geometry; a slice's is not");
    if (acc->has_samples)
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": the accumulator already holds samples; attach a shutter before the first render");
    if (s->live_accums != 1)
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": the scene has " + std::to_string(s->live_accums - 1) + " other live accumulator(s), whose sums are of one geometry");
    const uint32_t n = desc->n_triangles;
    if (n != 0 && n != s->dev.n_triangles)
        return rt::fail(RT_ERR_INVALID_ARG, FN + ": n_triangles is " + std::to_string(n) + ", the scene has " + std::to_string(s->dev.n_triangles) + " (or 0: the geometry does not move)");
    if (desc->sensor1) {
        if (desc->sensor1->kind != acc->sensor_desc.kind)
            return rt::fail(RT_ERR_INVALID_ARG, FN + ": sensor1 is of kind " + std::to_string(desc->sensor1->kind) + ", the accumulator's view of kind " + std::to_string(acc->sensor_desc.kind));
        if (int rc = rt::check_sensor(*desc->sensor1, acc->width, acc->height, FN.c_str()); rc != RT_OK)
            return rc;
    }
    rt::Shutter H;
    H.n = n, H.mode = desc->mode, H.slices = desc->slices, H.block = desc->block, H.open = desc->open, H.close = desc->close;
    if (desc->sensor1)
        H.has_sensor1 = true, H.sensor1 = *desc->sensor1;
    HIP_TRY(hipSetDevice(s->device));
    rt::DevArena arena; // the accumulator's only once nothing can be refused any more
    if (n) {
        const bool device = (desc->flags & RT_FLAG_DEVICE_FB) != 0;
        const size_t f9 = 36 * (size_t)n;
        if (device)
            for (int key = 0; key < 2; ++key) {
                rt_geometry_update u{};
                u.n_triangles = n;
                u.positions = desc->positions[key], u.normals = desc->normals[key], u.tangents = desc->tangents[key];
                u.texcoords = desc->texcoords, u.material_ids = desc->material_ids;
                if (int rc = rt::check_device_pointers(s, &u); rc != RT_OK)
                    return rc;
            }
        const std::vector<uint8_t> emissive = rt::emissive_materials(s->prep->mats);
        uint8_t *d_emissive = nullptr;
        uint32_t *d_moving = nullptr;
        auto alloc = [&]<class T>(T **p, size_t bytes) -> int {
            if (hipError_t e = arena.alloc_bytes(p, bytes); e != hipSuccess)
                return rt::hip_fail(e, FN);
            return RT_OK;
        };
        for (rt::ShutterArrays *arr : {&H.key[0], &H.key[1], &H.blend})
            for (float *&p : arr->a)
                if (int rc = alloc(&p, f9); rc != RT_OK)
                    return rc;
        int rc;
        if ((rc = alloc(&H.uv, 24 * (size_t)n)) != RT_OK || (rc = alloc(&H.mat, 4 * (size_t)n)) != RT_OK ||
            (rc = alloc(&d_emissive, std::max<size_t>(emissive.size(), 1))) != RT_OK || (rc = alloc(&d_moving, 4)) != RT_OK)
            return rc;
        // ---- the keys, host or device, to the accumulator's own copies: the call's one staging path
        rt::CallIo io(s->stream, s->staging, device);
        const float *src[2][3], *src_uv;
        const uint32_t *src_mat;
        for (int key = 0; key < 2; ++key) {
            io.in(&src[key][0], desc->positions[key], f9);
            io.in(&src[key][1], desc->normals[key], f9);
            io.in(&src[key][2], desc->tangents[key], f9);
        }
        io.in(&src_uv, desc->texcoords, 24 * (size_t)n);
        io.in(&src_mat, desc->material_ids, 4 * (size_t)n);
        uint32_t moving = 1;
        rc = io.run([&]() -> int {
            for (int key = 0; key < 2; ++key)
                for (int a = 0; a < 3; ++a)
                    HIP_TRY(hipMemcpyAsync(H.key[key].a[a], src[key][a], f9, hipMemcpyDeviceToDevice, s->stream));
            HIP_TRY(hipMemcpyAsync(H.uv, src_uv, 24 * (size_t)n, hipMemcpyDeviceToDevice, s->stream));
            HIP_TRY(hipMemcpyAsync(H.mat, src_mat, 4 * (size_t)n, hipMemcpyDeviceToDevice, s->stream));
            if (!emissive.empty())
                HIP_TRY(hipMemcpyAsync(d_emissive, emissive.data(), emissive.size(), hipMemcpyHostToDevice, s->stream));
            HIP_TRY(hipMemsetAsync(d_moving, 0, 4, s->stream));
            return RT_OK;
        });
        if (rc != RT_OK)
            return rc;
        // ---- what rt_update_geometry_device refuses of either key in this mode, before anything is written (the clamp keeps every slice
        // between the keys, so their finiteness and the upper end of the exponent range cover the slices)
        for (int key = 0; key < 2; ++key) {
            const rt_geometry_update u = update_of(H, H.key[key]);
            rt::UpdateScan scan;
            if ((rc = rt::refuse_device_arrays(s, &u, FN + " (key " + std::to_string(key) + ")", &scan)) != RT_OK)
                return rc;
        }
        // ---- static lights: ids are in range now
        rc = rt::queue_and_wait(s->stream, [&]() -> int {
            HIP_TRY(rt::launch_shutter_moving_lights(H.key[0].a[0], H.key[1].a[0], H.mat, d_emissive, (uint32_t)emissive.size(), n, d_moving, s->stream));
            HIP_TRY(hipMemcpyAsync(&moving, d_moving, 4, hipMemcpyDeviceToHost, s->stream));
            return RT_OK;
        });
        if (rc != RT_OK)
            return rc;
        H.static_lights = moving == 0;
    }
    // ---- the scene becomes key 0's (the first write to anything a render kernel reads; a refusal of the update path leaves it as it was)
    acc->shutter = H;
    if (int rc = rt::shutter_install(acc, -1, /*keep_static_lights=*/false); rc != RT_OK) {
        acc->shutter.reset();
        return rc;
    }
    acc->owned.adopt(arena);
    ++s->shutter_accums;
    return RT_OK;
}

extern "C" int rt_accum_shutter_times(rt_accum *acc, double *slice_change_ms, uint32_t *slice_changes) {
    if (!acc || !slice_change_ms || !slice_changes || !acc->shutter)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_shutter_times: null argument, or the accumulator has no shutter (rt_accum_attach_shutter)");
    *slice_change_ms = acc->shutter->change_ms;
    *slice_changes = acc->shutter->changes;
    return RT_OK;
}

extern "C" int rt_accum_shutter_info(rt_accum *acc, uint32_t *static_lights, uint32_t *light_rebuilds) {
    if (!acc || !static_lights || !light_rebuilds || !acc->shutter)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_shutter_info: null argument, or the accumulator has no shutter (rt_accum_attach_shutter)");
    *static_lights = acc->shutter->static_lights ? 1u : 0u;
    *light_rebuilds = acc->shutter->light_rebuilds;
    return RT_OK;
}
