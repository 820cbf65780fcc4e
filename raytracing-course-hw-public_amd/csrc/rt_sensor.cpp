// rt_sensor.cpp — the cameras of the wavefront pipeline on the host (rt_abi.h rt_sensor; a view of rt_render* and the camera of
// rt_accum_create are pinhole records): the argument checks, the one place that fills a sensor record (make_sensor), rt_render_sensors*
// (rt_render.cpp render_image over its table, under the scene's policy for sensors of that kind) and rt_sensor_rays.
// rt_accum_create_sensor is in rt_accum_host.cpp.
#include <cmath>
#include <cstddef>
#include <cstring>

#include "rt_scene_impl.h"

// What every entry point refuses of a sensor at a width x height image (`fn`: its name). Needs no device.
int rt::check_sensor(const rt_sensor &sn, uint32_t width, uint32_t height, const char *fn) {
    const std::string name(fn);
    if (sn.kind > RT_SENSOR_THIN_LENS)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": unknown sensor kind " + std::to_string(sn.kind));
    for (uint32_t r : sn.reserved)
        if (r != 0)
            return rt::fail(RT_ERR_INVALID_ARG, name + ": reserved words of rt_sensor must be 0");
    if (sn.kind == RT_SENSOR_ORTHOGRAPHIC && !(std::isfinite(sn.half_width) && sn.half_width > 0.0f))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": an orthographic sensor needs a finite half_width > 0");
    if (sn.kind == RT_SENSOR_THIN_LENS && (!(std::isfinite(sn.lens_radius) && sn.lens_radius >= 0.0f) || !(std::isfinite(sn.focus_distance) && sn.focus_distance > 0.0f)))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": a thin-lens sensor needs a finite lens_radius >= 0 and a finite focus_distance > 0");
    if (sn.kind == RT_SENSOR_FISHEYE) {
        // the angle off axis is r * half_fov with r up to the corner's sqrt(1 + (H/W)^2): it must stay a valid sine argument and a live pixel
        const float half_fov = sn.camera.fov_x / 2;
        const double aspect = width ? (double)height / (double)width : 0.0;
        if (!(std::isfinite(half_fov) && half_fov > 0.0f) || (double)half_fov * std::sqrt(1.0 + aspect * aspect) > 3.14159265358979323846)
            return rt::fail(RT_ERR_INVALID_ARG, name + ": a fisheye sensor needs fov_x > 0 and a corner at most 180 degrees off axis: (fov_x / 2) * sqrt(1 + (H/W)^2) <= pi");
    }
    return RT_OK;
}

// The sensor record of one rt_sensor at a width x height image: the camera, gen_ray's tan terms (raytracer.h:531-535) and Camera::fov_y
// (scene.h:69-71) as float overloads, the seed, the kind and its hoisted terms. The one place every render, every view of rt_render_views
// and every accumulator take them from, so that view v of a batch gets the bits a scene created with its camera gets.
WfSensor rt::make_sensor(const rt_sensor &sn, uint32_t width, uint32_t height) {
    const rt_camera &cam = sn.camera;
    WfSensor r{};
    std::memcpy(r.pos, cam.position, 12);
    std::memcpy(r.right, cam.right, 12);
    std::memcpy(r.up, cam.up, 12);
    std::memcpy(r.fwd, cam.forward, 12);
    r.tan_x = std::tan(cam.fov_x / 2);
    const float fov_y = std::atan(std::tan(cam.fov_x / 2) * height / width) * 2;
    r.tan_y = std::tan(fov_y / 2);
    r.seed = sn.seed;
    r.kind = sn.kind;
    r.half_fov = cam.fov_x / 2;
    r.half_width = sn.half_width;
    r.half_h = sn.half_width * (float)height / (float)width;
    r.lens_radius = sn.lens_radius;
    r.focus_distance = sn.focus_distance;
    return r;
}
// the pinhole record of a view {camera, seed}
WfSensor rt::make_sensor(const rt_camera &cam, uint64_t seed, uint32_t width, uint32_t height) {
    rt_sensor sn{};
    sn.camera = cam;
    sn.kind = RT_SENSOR_PINHOLE;
    sn.seed = seed;
    return rt::make_sensor(sn, width, height);
}

// The one origin of every ray of a pass over `table`, where it has one: a single camera of a kind whose rays all start at the camera
// position, bit for bit. Their packets may walk the camera-relative records (rt_kernels.h WfPassKind::relative_origin). Null otherwise.
const float *rt::single_origin(const WfSensor *table, uint32_t n) {
    const bool at_pos = n == 1 && (table[0].kind == RT_SENSOR_PINHOLE || table[0].kind == RT_SENSOR_EQUIRECT || table[0].kind == RT_SENSOR_FISHEYE);
    return at_pos ? table[0].pos : nullptr;
}

static int render_sensors_impl(rt_scene *s, const rt_params *p, const rt_sensor *sensors, uint32_t n_sensors, float *fb_rgb, uint8_t *rgb8, rt_stats *stats, const char *fn) {
    const std::string name(fn);
    if (!s || !p || !sensors || n_sensors == 0 || (!fb_rgb && !rgb8))
        return rt::fail(RT_ERR_INVALID_ARG, name + ": null argument or no sensor");
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, name + ": sensors render on single-GPU scenes only");
    if (int rc = rt::check_wavefront_entry(p, fn, "sensors", RT_FLAG_DEVICE_FB | RT_FLAG_COUNTERS | RT_FLAG_MEGAKERNEL | RT_FLAG_GLOBAL_BEST, true); rc != RT_OK)
        return rc;
    if (p->width == 0 || p->height == 0 || (uint64_t)n_sensors * p->width * p->height >= 0x7FFFFFFFull)
        return rt::fail(RT_ERR_INVALID_ARG, name + ": the image is empty, or n_sensors x width x height reaches 2^31");
    for (uint32_t v = 0; v < n_sensors; ++v)
        if (int rc = rt::check_sensor(sensors[v], p->width, p->height, fn); rc != RT_OK)
            return rc;
    std::vector<WfSensor> table(n_sensors);
    for (uint32_t v = 0; v < n_sensors; ++v)
        table[v] = rt::make_sensor(sensors[v], p->width, p->height);
    // The policy: one per kind for a single sensor, [5] for several
    return rt::render_image(s, p, table, s->pkt_sensor[n_sensors == 1 ? table[0].kind : 5u], fb_rgb, rgb8, stats);
}

extern "C" int rt_render_sensors(rt_scene *s, const rt_params *p, const rt_sensor *sensors, uint32_t n_sensors, float *fb_rgb, rt_stats *stats) {
    if (!fb_rgb)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_render_sensors: null argument");
    return render_sensors_impl(s, p, sensors, n_sensors, fb_rgb, nullptr, stats, "rt_render_sensors");
}

extern "C" int rt_render_sensors_rgb8(rt_scene *s, const rt_params *p, const rt_sensor *sensors, uint32_t n_sensors, uint8_t *rgb8, rt_stats *stats) {
    if (!rgb8)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_render_sensors_rgb8: null argument");
    return render_sensors_impl(s, p, sensors, n_sensors, nullptr, rgb8, stats, "rt_render_sensors_rgb8");
}

extern "C" int rt_sensor_rays(rt_scene *s, const rt_sensor *sensor, uint32_t width, uint32_t height, uint32_t first_pixel, uint32_t n_pixels, uint32_t first_sample,
                              uint32_t samples, uint32_t flags, rt_ray *rays_out) {
    if (!s || !sensor)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_sensor_rays: null argument");
    if (s->group)
        return rt::fail(RT_ERR_UNSUPPORTED, "rt_sensor_rays: sensors are evaluated on single-GPU scenes only");
    if (flags & ~(uint32_t)RT_FLAG_DEVICE_FB)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_sensor_rays: flags other than RT_FLAG_DEVICE_FB");
    if (width == 0 || height == 0 || (uint64_t)width * height >= 0x7FFFFFFFull)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_sensor_rays: image size " + std::to_string(width) + "x" + std::to_string(height));
    if ((uint64_t)first_pixel + n_pixels > (uint64_t)width * height)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_sensor_rays: the pixel range ends past width x height");
    const uint64_t n = (uint64_t)n_pixels * samples;
    if (n >= 0x80000000ull)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_sensor_rays: n_pixels x samples must stay below 2^31");
    if (int rc = rt::check_sensor(*sensor, width, height, "rt_sensor_rays"); rc != RT_OK)
        return rc;
    if (n == 0)
        return RT_OK;
    const bool device_out = (flags & RT_FLAG_DEVICE_FB) != 0;
    if (!rays_out || (device_out && (reinterpret_cast<uintptr_t>(rays_out) & 15u) != 0))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_sensor_rays: null output, or a device buffer that is not 16-byte aligned");
    HIP_TRY(hipSetDevice(s->device));
    const WfSensor rec = rt::make_sensor(*sensor, width, height);
    if (int rc = s->ensure_sensors(1); rc != RT_OK)
        return rc;
    rt::CallIo io(s->stream, s->staging, device_out);
    rt_ray *d_out;
    io.out(&d_out, rays_out, (size_t)n * sizeof(rt_ray));
    return io.run([&]() -> int {
        HIP_TRY(hipMemcpyAsync(s->sensors.get(), &rec, sizeof(rec), hipMemcpyHostToDevice, s->stream)); // `rec` outlives the bracket's wait
        HIP_TRY(rt::launch_sensor_rays(s->sensors.get(), width, height, first_pixel, first_sample, samples, (uint32_t)n, d_out, s->num_cus, s->stream));
        return RT_OK;
    });
}
