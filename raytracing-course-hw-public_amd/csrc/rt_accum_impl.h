// rt_accum_impl.h — what the two host files of the accumulators share (internal): the definition of rt_accum and the helpers with more
// than one user. rt_accum_host.cpp creates, renders, resolves and reads an accumulator; rt_accum_layers.cpp holds its optional layers (first-hit
// features with the denoiser, ids, light groups) and rt_accum_flow.cpp the fourth (motion vectors), each with its attach / read / resolve
// entry points. DESIGN.md "accumulator layers" lists what a layer consists of.
#pragma once
#include <optional>

#include "rt_scene_impl.h"
#include "rt_shutter.h"

namespace rt {
// rt_accum_attach_shutter's layer (rt_accum_shutter.cpp): the two keys and the scratch triple on the device, the second view, the call's
// bookkeeping. Unlike the other layers it adds no sums: it decides which scene and which view a sample is rendered with.
struct Shutter {
    uint32_t n = 0;                  // triangles of the keys; 0: the geometry does not move
    uint32_t mode = RT_UPDATE_REBUILD, slices = 1, block = 1;
    float open = 0.0f, close = 1.0f;
    ShutterArrays key[2], blend;     // positions / normals / tangents of key 0, key 1 and of the slice being rendered
    float *uv = nullptr;             // not interpolated
    uint32_t *mat = nullptr;
    bool static_lights = false;      // no emissive triangle's position keys differ in a bit: every slice's light tree is key 0's
    bool has_sensor1 = false;
    rt_sensor sensor1{};
    uint64_t n_samples = 0;          // n: the samples every pixel holds
    double change_ms = 0;            // rt_accum_shutter_times: the slice installs of the last render call ...
    uint32_t changes = 0;            // ... and how many there were
    uint32_t light_rebuilds = 0;     // installs since attach (slices and key 0) that built a light tree
};
} // namespace rt

struct rt_accum {
    rt_scene *scene = nullptr;
    uint32_t width = 0, height = 0;
    WfSensor sensor{};            // its camera: rt_accum_create_sensor's, or the pinhole record of {camera, seed} (host copy of d_sensor)
    WfSensor *d_sensor = nullptr; // WfLaunch::sensors of its passes: the one record
    rt_sensor sensor_desc{};      // what `sensor` was made of: the view at t = 0 of a shutter
    rt::AccumRound R{};
    rt::DevArena owned{16};
    rt::PacketPolicy pkt; // of its own passes, kept apart from rt_render's
    // The optional layers: a record is there exactly when the accumulator keeps the layer. Its sums and tables are the accumulator's; its
    // per-path records (rec, tag) are the scene's, bound per fill (rt_scene::bind_layer_records).
    std::optional<WfFeat> features; // RT_ACCUM_FEATURES: the four first-hit sums
    std::optional<WfIds> ids;       // rt_accum_attach_ids: the per-pixel id tables
    std::optional<WfGroups> groups; // rt_accum_attach_light_groups: the group sums and the material table
    std::optional<WfFlow> flow;     // rt_accum_attach_flow: the four flow values per pixel, the two keys and the second view
    std::optional<rt::Shutter> shutter; // rt_accum_attach_shutter: the keys (no sums of its own)
    rt::DenoiseBufs D{};            // rt_accum_denoise's workspace (64 B per pixel), allocated by its first call
    rt::DevBuf<uint32_t> matte_set; // rt_accum_resolve_matte's id set on the device
    bool has_samples = false; // a call has queued a pass of this accumulator: ids and light groups can no longer be attached
    ~rt_accum() {
        (void)hipSetDevice(scene->device);
        (void)hipStreamSynchronize(scene->stream); // `owned` frees after this body: on this device, behind this synchronise
        if (counted)
            --scene->live_accums;
        if (shutter)
            --scene->shutter_accums;
    }
    bool counted = false; // it is one of scene->live_accums
};

namespace rt {
template <class T> T *layer_ptr(std::optional<T> &layer) { return layer ? &*layer : nullptr; }

template <class T> int accum_alloc(rt_accum *a, size_t bytes, T **ptr, const char *fn) {
    if (hipError_t e = a->owned.alloc_bytes(ptr, bytes); e != hipSuccess)
        return hip_fail(e, fn);
    return RT_OK;
}

// The entry check of a call on a live accumulator: it is there, and it keeps the layer the call reads.
enum class AccumNeed { NONE, FEATURES, IDS, GROUPS, FLOW };
inline int accum_entry(const rt_accum *acc, const char *fn, AccumNeed need) {
    if (!acc)
        return fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null accumulator");
    if (need == AccumNeed::FEATURES && !acc->features)
        return fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the accumulator was created without RT_ACCUM_FEATURES");
    if (need == AccumNeed::IDS && !acc->ids)
        return fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the accumulator has no ids (rt_accum_attach_ids)");
    if (need == AccumNeed::GROUPS && !acc->groups)
        return fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the accumulator has no light groups (rt_accum_attach_light_groups)");
    if (need == AccumNeed::FLOW && !acc->flow)
        return fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the accumulator has no flow (rt_accum_attach_flow)");
    return RT_OK;
}
// rt_accum_shutter.cpp: the scene and the accumulator's view at slice k of its shutter (k < 0: key 0 and the accumulator's own view, what every
// call leaves behind), and the slice of sample index s
int shutter_install(rt_accum *a, int k, bool keep_static_lights = true);
uint32_t shutter_slice(const Shutter &H, uint64_t s);
// "flags other than RT_FLAG_DEVICE_FB": the one flag an accumulator's reads and tables take
inline bool other_flags(uint32_t flags) { return (flags & ~(uint32_t)RT_FLAG_DEVICE_FB) != 0; }

// the accumulator's own arrays, each to a host destination that is not null
struct ReadBack {
    void *host;
    const void *dev;
    size_t bytes;
};
inline int read_back(rt_accum *acc, std::initializer_list<ReadBack> list) {
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    return queue_and_wait(s->stream, [&]() -> int {
        for (const ReadBack &r : list)
            if (r.host)
                HIP_TRY(hipMemcpyAsync(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost, s->stream));
        return RT_OK;
    });
}

// An image of an accumulator is a callable hipError_t image(float *d_fb) that fills width x height x 3 floats on the device. accum_image
// delivers it to a float destination, or through the film (image.h:49-82, as rt_render_rgb8) to an rgb8 one; host or HBM by `flags`.
template <class Image> int accum_image(rt_accum *acc, uint32_t flags, float *fb_rgb, Image image) {
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    float *d_fb;
    io.out(&d_fb, fb_rgb, (size_t)acc->width * acc->height * 12);
    return io.run([&]() -> int {
        HIP_TRY(image(d_fb));
        return RT_OK;
    });
}
template <class Image> int accum_image(rt_accum *acc, uint32_t flags, uint8_t *rgb8, Image image) {
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = s->ensure_film(); rc != RT_OK)
        return rc;
    const uint32_t n = acc->width * acc->height;
    CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    float *d_fb;
    uint8_t *d_rgb8;
    io.scratch(&d_fb, 12ull * n);
    io.out(&d_rgb8, rgb8, 3ull * n);
    return io.run([&]() -> int {
        HIP_TRY(image(d_fb));
        HIP_TRY(launch_film(d_fb, d_rgb8, n, 0, 1, n, s->film_table.get(), s->stream));
        return RT_OK;
    });
}
} // namespace rt
