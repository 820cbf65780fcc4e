// main.cpp — host driver behind the reference's CLI:  run.sh <scene.gltf | scene.txt> <W> <H> <SPP> <out.ppm>
// Restates src/main.cpp:16-49: parse 5 positional arguments, load the scene, render, tone-map, write the PPM.
// The only change of substance is line 37 of the reference: run_raytracer(scene, img) becomes
// rt_create + rt_render_rgb8 through the C ABI (include/rt_abi.h): render and film (image.h) on the device.
// Optional environment: RT_DEVICE (HIP ordinal; unset = every visible GPU: replicas + RCCL gather inside the library, the
// node-scale counterpart of the thread pool of raytracer.h:636-665), RT_RNG_MODE (device|reference), RT_SEED,
// RT_ENV_MAP (+ RT_ENV_MAP_INTENSITY): the environment map the reference enables at compile time (config.h:36-38, main.cpp:28-31);
// RT_ENV_RADIANCE=1 (with RT_ENV_MAP): the map lights the scene as float radiance (rt_set_environment after rt_create, on one GPU): an .hdr
// keeps the values the 8-bit load clips to [0, 1]; RT_ENV_IMPORTANCE=1 adds RT_ENV_IMPORTANCE, which importance-samples it.
// RT_LIGHT_TRIANGLE=1 (+ RT_LIGHT_TRIANGLE_INTENSITY): its extra light source in camera coordinates (config.h:40-47, scene.h:479-498).
// Tuning (the library itself reads NO environment variable since ABI 4; this file translates them into rt_scene_desc / rt_params
// fields): RT_BVH_DEVICE=1, RT_BVH_WIDE=1 (production builds), RT_TRAVERSAL=global, RT_WF_SORT=<0|5> (off | sorted), RT_WF_PACKET=<0|1>,
// RT_WF_MAX_PATHS=<n>, RT_DEVICE_BUILDER=lbvh, RT_PLOC_RADIUS=<n>. RT_VERBOSE: the reference's progress line "%d/%d     \r"
// (raytracer.h:647) per finished pass, and a timing line on stderr.
// RT_ALL_CAMERAS=1: render EVERY camera of the file (rt_loaded_cameras; the reference keeps only the last) in one rt_render_views_rgb8
// call, all with RT_SEED, and write camera i to <stem>_<i><ext> of the output path.
// RT_ADAPTIVE=<threshold>: adaptive sampling through an accumulator (rt_accum_render_adaptive) of the scene's camera on one GPU; the SPP
// argument becomes max_samples, RT_ADAPTIVE_MIN (default 16, capped at the SPP) and RT_ADAPTIVE_STEP (default 32) set min_samples and step.
// RT_SPP_MAP=<file.pgm> also writes the per-pixel sample counts (16-bit PGM). RT_VERBOSE adds the rounds and the mean SPP.
// RT_DENOISE=1: render through a feature accumulator (rt_accum_create_ex, RT_ACCUM_FEATURES) on one GPU and write the image filtered by
// rt_accum_denoise (defaults of rt_denoise); with RT_ADAPTIVE the samples come from the adaptive call, otherwise the SPP argument is one
// progressive call (rt_accum_render). RT_AOV=<prefix> (with or without RT_DENOISE: it renders through a feature accumulator too) also writes
// the first-hit feature means: <prefix>_albedo.ppm (clamp(a, 0, 1) * 255 + 0.5, truncated), <prefix>_normal.ppm (0.5 * n + 0.5, quantised
// likewise) and <prefix>_depth.pfm (one channel "Pf", little-endian floats, rows bottom to top as PFM has them).
// RT_LIGHT_GROUPS=material: render through an accumulator with light groups (rt_accum_attach_light_groups) on one GPU: every emissive material
// (a non-zero emission factor, the library's own test) is a group of its own, in material order, and the background is the last group; more
// than RT_LIGHT_GROUP_MAX groups are refused with a message. Besides the image it writes each group alone (rt_accum_resolve_light_group through
// the film) to <stem>_group_<g><ext> of the output path.
// RT_CAMERA=pinhole|equirect|fisheye|ortho|thinlens: render the file's camera through a sensor model evaluated on the device (rt_abi.h
// rt_sensor), on one GPU, with RT_SEED as its seed: rt_render_sensors_rgb8, or rt_accum_create_sensor where RT_ADAPTIVE / RT_DENOISE / RT_AOV ask
// for an accumulator. RT_CAMERA_FOV_DEG replaces the camera's horizontal field of view (pinhole, fisheye, thinlens); RT_ORTHO_HALF_WIDTH
// (default 1), RT_LENS_RADIUS (default 0) and RT_FOCUS_DISTANCE (default 1) are the sensor's fields. Unset: exactly the path above.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/rt_abi.h"
#include "../../../include/rt_host.h"

static void print_progress(uint32_t done, uint32_t total, void *) {
    std::printf("%d/%d     \r", (int)done, (int)total); // raytracer.h:647 (there: spans; here: passes)
    std::fflush(stdout);
}

static int die(const char *what) {
    std::cerr << what << ": " << rt_last_error() << std::endl; // main.cpp:46-49
    return EXIT_FAILURE;
}

int main(int argc, char **argv) {
    if (argc < 6) {
        std::cerr << "Too few arguments: expected 6, got " << argc - 1 << std::endl; // main.cpp:17-21 (sic)
        return EXIT_FAILURE;
    }
    unsigned width = std::strtol(argv[2], nullptr, 10);
    unsigned height = std::strtol(argv[3], nullptr, 10);
    unsigned samples = std::strtol(argv[4], nullptr, 10);
    if ((int)width <= 0 || (int)height <= 0) { // Image ctor image.h:25-29
        std::cerr << "Illegal image size" << (int)width << "x" << (int)height << std::endl;
        return EXIT_FAILURE;
    }
    rt_loaded_scene *loaded = nullptr;
    // *.txt: the scene-txt front end (BASELINE configs 1-2; no parser at the reference's HEAD), anything else: glTF (main.cpp:27)
    if (rt_scene_load(argv[1], static_cast<float>(width) / height, &loaded) != RT_OK)
        return die("load");
    auto env_on = [](const char *name) {
        const char *v = std::getenv(name);
        return v && std::atoi(v) != 0;
    };
    const char *env_radiance = env_on("RT_ENV_RADIANCE") ? std::getenv("RT_ENV_MAP") : nullptr; // the map as float radiance, set after rt_create
    if (const char *env_map = env_radiance ? nullptr : std::getenv("RT_ENV_MAP")) { // USE_ENV_MAP / ENV_MAP_PATH / ENV_MAP_INTENSITY, config.h:36-38
        const char *k = std::getenv("RT_ENV_MAP_INTENSITY");
        if (rt_loaded_set_env_map(loaded, env_map, k ? std::strtof(k, nullptr) : 1.0f) != RT_OK) {
            rt_loaded_free(loaded);
            return die("environment map");
        }
    }
    if (const char *ut = std::getenv("RT_USE_TEXTURES"); ut && std::atoi(ut) == 0) // USE_TEXTURES = false, config.h:31-32
        rt_loaded_disable_textures(loaded);
    if (const char *lt = std::getenv("RT_LIGHT_TRIANGLE"); lt && std::atoi(lt) != 0) { // ADD_LIGHT_TRIANGLE / LIGHT_TRIANGLE_* of config.h:40-47
        const float rel[9] = {10, 0, -0.1f, 0, 10, -0.1f, 0, -10, -0.1f};
        const char *k = std::getenv("RT_LIGHT_TRIANGLE_INTENSITY");
        if (rt_loaded_add_light_triangle(loaded, rel, k ? std::strtof(k, nullptr) : 10.0f) != RT_OK) {
            rt_loaded_free(loaded);
            return die("light triangle");
        }
    }
    const char *dev_env = std::getenv("RT_DEVICE");
    const char *adaptive = std::getenv("RT_ADAPTIVE"); // accumulators run on one GPU
    const bool denoise = env_on("RT_DENOISE");
    const char *aov = std::getenv("RT_AOV");
    const char *light_groups = std::getenv("RT_LIGHT_GROUPS");
    const bool accumulate = adaptive || denoise || aov || light_groups;
    const char *camera_kind = std::getenv("RT_CAMERA"); // sensors are evaluated on one GPU
    rt_scene *scene = nullptr;
    const int device = dev_env ? std::atoi(dev_env) : (rt_device_count() > 1 && !accumulate && !camera_kind && !env_radiance ? RT_ALL_DEVICES : 0);
    rt_scene_desc desc = *rt_loaded_desc(loaded); // the arrays stay the loader's; only the build options change
    if (env_on("RT_BVH_DEVICE"))
        desc.build_flags |= RT_BUILD_DEVICE_LBVH;
    if (env_on("RT_BVH_WIDE"))
        desc.build_flags |= RT_BUILD_WIDE;
    if (const char *b = std::getenv("RT_DEVICE_BUILDER"); b && !std::strcmp(b, "lbvh"))
        desc.build.device_builder = RT_BUILDER_LBVH;
    if (const char *r = std::getenv("RT_PLOC_RADIUS"))
        desc.build.ploc_radius = (uint32_t)std::atoi(r);
    if (env_radiance) { // bg_color = intensity, as rt_loaded_set_env_map sets it for the 8-bit map (main.cpp:28)
        const char *k = std::getenv("RT_ENV_MAP_INTENSITY");
        desc.bg_color[0] = desc.bg_color[1] = desc.bg_color[2] = k ? std::strtof(k, nullptr) : 1.0f;
    }
    std::vector<uint32_t> material_group; // RT_LIGHT_GROUPS=material: the group of every material, then n_groups with the background last
    uint32_t n_groups = 0;
    if (light_groups) {
        if (std::strcmp(light_groups, "material") != 0) {
            rt_loaded_free(loaded);
            std::cerr << "RT_LIGHT_GROUPS: material (one group per emissive material, the background last)" << std::endl;
            return EXIT_FAILURE;
        }
        material_group.assign(desc.n_materials, RT_LIGHT_GROUP_NONE);
        for (uint32_t i = 0; i < desc.n_materials; ++i) {
            const float *e = desc.materials[i].emission;
            if (!((e[0] == 0) & (e[1] == 0) & (e[2] == 0)))
                material_group[i] = n_groups++;
        }
        n_groups += 1; // the background
        if (n_groups > RT_LIGHT_GROUP_MAX) {
            rt_loaded_free(loaded);
            std::cerr << "RT_LIGHT_GROUPS=material: " << n_groups - 1 << " emissive materials and the background make " << n_groups << " groups; at most "
                      << RT_LIGHT_GROUP_MAX << " are kept" << std::endl;
            return EXIT_FAILURE;
        }
    }
    int crc = rt_create(&desc, device, &scene);
    if (crc == RT_ERR_COMM && device == RT_ALL_DEVICES) {
        // the multi-GPU group could not be formed (librccl missing, or it refuses this device set): one GPU still renders
        std::cerr << "rt_create: " << rt_last_error() << "; falling back to GPU 0 (set RT_DEVICE to choose another)" << std::endl;
        crc = rt_create(&desc, 0, &scene);
    }
    if (crc != RT_OK) {
        rt_loaded_free(loaded);
        return die("rt_create");
    }
    if (env_radiance) {
        rt_environment env{};
        float *texels = nullptr;
        int erc = rt_image_decode_radiance(env_radiance, &env.width, &env.height, &texels);
        env.rgb = texels;
        env.flags = env_on("RT_ENV_IMPORTANCE") ? RT_ENV_IMPORTANCE : 0u;
        if (erc == RT_OK)
            erc = rt_set_environment(scene, &env);
        rt_free(texels);
        if (erc != RT_OK) {
            rt_destroy(scene);
            rt_loaded_free(loaded);
            return die("environment map");
        }
    }
    rt_params p{};
    p.width = width;
    p.height = height;
    p.samples = samples;
    const char *mode = std::getenv("RT_RNG_MODE");
    p.rng_mode = (mode && !std::strcmp(mode, "reference")) ? RT_RNG_REFERENCE : RT_RNG_DEVICE;
    const char *seed = std::getenv("RT_SEED");
    p.seed = seed ? std::strtoull(seed, nullptr, 0) : 0;
    if (const char *t = std::getenv("RT_TRAVERSAL"); t && !std::strcmp(t, "global"))
        p.flags |= RT_FLAG_GLOBAL_BEST;
    if (const char *v = std::getenv("RT_WF_SORT"))
        p.sort_mode = (uint32_t)std::atoi(v) + 1u; // RT_SORT_OFF = 1, RT_SORT_OCTANT_CELL_CONE = 6
    if (const char *v = std::getenv("RT_WF_PACKET"))
        p.packet_mode = std::atoi(v) ? RT_PACKET_ON : RT_PACKET_OFF;
    if (const char *v = std::getenv("RT_WF_MAX_PATHS"))
        p.max_paths = std::strtoull(v, nullptr, 0);
    const bool verbose = std::getenv("RT_VERBOSE") != nullptr;
    if (verbose)
        p.progress = print_progress;
    // Image::set_pixel tone-maps as pixels finish (image.h:40-42): the film runs on the device too, unless the host
    // film is asked for (RT_FILM=host) or the device film declines (RT_ERR_UNSUPPORTED: libm failed its self-check)
    std::vector<rt_view> views; // RT_ALL_CAMERAS: one view per camera of the file; empty: the plain render of the scene's camera
    if (env_on("RT_ALL_CAMERAS")) {
        uint32_t n_cams = 0;
        rt_loaded_cameras(loaded, nullptr, 0, &n_cams);
        std::vector<rt_camera> cams(n_cams);
        rt_loaded_cameras(loaded, cams.data(), n_cams, &n_cams);
        if (cams.empty())
            cams.push_back(desc.camera);
        for (const rt_camera &c : cams) {
            rt_view v{};
            v.camera = c;
            v.seed = p.seed;
            views.push_back(v);
        }
    }
    const size_t n_out = views.empty() ? 1 : views.size();
    const size_t view_pixels = (size_t)width * height;
    std::vector<uint8_t> rgb8(n_out * view_pixels * 3, 0);
    rt_stats st{};
    const char *film = std::getenv("RT_FILM");
    int rc = RT_ERR_UNSUPPORTED;
    rt_sensor sensor{};
    if (camera_kind) {
        static const char *const names[] = {"pinhole", "equirect", "fisheye", "ortho", "thinlens"};
        uint32_t kind = 0;
        while (kind < 5 && std::strcmp(camera_kind, names[kind]) != 0)
            ++kind;
        if (kind == 5 || !views.empty() || p.rng_mode != RT_RNG_DEVICE) {
            rt_destroy(scene);
            rt_loaded_free(loaded);
            std::cerr << "RT_CAMERA: pinhole, equirect, fisheye, ortho or thinlens; the scene's camera only (not with RT_ALL_CAMERAS), device RNG only" << std::endl;
            return EXIT_FAILURE;
        }
        sensor.camera = desc.camera;
        if (const char *v = std::getenv("RT_CAMERA_FOV_DEG"))
            sensor.camera.fov_x = std::strtof(v, nullptr) * (3.14159265358979323846f / 180.0f);
        sensor.kind = kind;
        const char *hw = std::getenv("RT_ORTHO_HALF_WIDTH"), *lr = std::getenv("RT_LENS_RADIUS"), *fd = std::getenv("RT_FOCUS_DISTANCE");
        sensor.half_width = hw ? std::strtof(hw, nullptr) : 1.0f;
        sensor.lens_radius = lr ? std::strtof(lr, nullptr) : 0.0f;
        sensor.focus_distance = fd ? std::strtof(fd, nullptr) : 1.0f;
        sensor.seed = p.seed;
    }
    uint32_t rounds = 0;
    std::vector<uint32_t> spp_map;
    std::vector<float> aov_albedo, aov_normal, aov_depth;
    std::vector<uint8_t> group_rgb8; // RT_LIGHT_GROUPS: n_groups images
    if (accumulate) {
        if (!views.empty()) {
            rt_destroy(scene);
            rt_loaded_free(loaded);
            std::cerr << "RT_ADAPTIVE / RT_DENOISE / RT_AOV / RT_LIGHT_GROUPS render the scene's camera only (not with RT_ALL_CAMERAS)" << std::endl;
            return EXIT_FAILURE;
        }
        rt_accum *acc = nullptr;
        const uint32_t accum_flags = (denoise || aov) ? RT_ACCUM_FEATURES : 0u;
        rc = camera_kind ? rt_accum_create_sensor(scene, width, height, &sensor, accum_flags, &acc) : rt_accum_create_ex(scene, width, height, nullptr, p.seed, accum_flags, &acc);
        if (rc == RT_OK && light_groups) {
            rt_light_group_desc lg{};
            lg.n_groups = n_groups;
            lg.background_group = n_groups - 1;
            lg.material_group = material_group.data();
            lg.n_materials = desc.n_materials;
            rc = rt_accum_attach_light_groups(acc, &lg);
        }
        if (rc == RT_OK && adaptive) {
            rt_adaptive ad{};
            ad.threshold = std::strtof(adaptive, nullptr);
            ad.max_samples = samples;
            const char *mn = std::getenv("RT_ADAPTIVE_MIN");
            ad.min_samples = mn ? (uint32_t)std::strtoul(mn, nullptr, 10) : std::min(16u, samples);
            if (const char *step = std::getenv("RT_ADAPTIVE_STEP"))
                ad.step = (uint32_t)std::strtoul(step, nullptr, 10);
            rc = rt_accum_render_adaptive(acc, &p, &ad, &rounds, &st);
        } else if (rc == RT_OK) {
            rc = rt_accum_render(acc, &p, &st); // the SPP argument as one progressive call
        }
        if (rc == RT_OK) { // the film as for rt_render_rgb8: on the device unless RT_FILM=host or the device film declines
            const bool host_film = film && !std::strcmp(film, "host");
            rc = host_film ? RT_ERR_UNSUPPORTED : denoise ? rt_accum_denoise_rgb8(acc, nullptr, 0, rgb8.data()) : rt_accum_resolve_rgb8(acc, 0, rgb8.data());
            if (rc == RT_ERR_UNSUPPORTED) {
                std::vector<float> fb(view_pixels * 3, 0.0f);
                rc = denoise ? rt_accum_denoise(acc, nullptr, 0, fb.data()) : rt_accum_resolve(acc, 0, fb.data());
                if (rc == RT_OK)
                    rt_tonemap_rgb8(fb.data(), view_pixels, rgb8.data());
            }
        }
        if (rc == RT_OK && light_groups) { // each group alone, through the same film as the image
            group_rgb8.resize((size_t)n_groups * view_pixels * 3);
            std::vector<float> fb(view_pixels * 3, 0.0f);
            for (uint32_t g = 0; g < n_groups && rc == RT_OK; ++g) {
                rc = rt_accum_resolve_light_group(acc, g, 0, fb.data());
                if (rc == RT_OK)
                    rt_tonemap_rgb8(fb.data(), view_pixels, group_rgb8.data() + (size_t)g * view_pixels * 3);
            }
        }
        if (rc == RT_OK && adaptive) {
            spp_map.resize(view_pixels);
            rc = rt_accum_read(acc, nullptr, nullptr, spp_map.data(), nullptr);
        }
        if (rc == RT_OK && aov) {
            aov_albedo.resize(view_pixels * 3), aov_normal.resize(view_pixels * 3), aov_depth.resize(view_pixels);
            rc = rt_accum_resolve_features(acc, 0, aov_albedo.data(), aov_normal.data(), aov_depth.data());
        }
        if (acc)
            rt_accum_destroy(acc);
    } else if (camera_kind) {
        rc = (film && !std::strcmp(film, "host")) ? RT_ERR_UNSUPPORTED : rt_render_sensors_rgb8(scene, &p, &sensor, 1, rgb8.data(), &st);
        if (rc == RT_ERR_UNSUPPORTED) { // RT_FILM=host, or the device film declined: the float image and the host film
            std::vector<float> fb(view_pixels * 3, 0.0f);
            rc = rt_render_sensors(scene, &p, &sensor, 1, fb.data(), &st);
            if (rc == RT_OK)
                rt_tonemap_rgb8(fb.data(), view_pixels, rgb8.data());
        }
    } else if (!(film && !std::strcmp(film, "host")))
        rc = views.empty() ? rt_render_rgb8(scene, &p, rgb8.data(), &st) : rt_render_views_rgb8(scene, &p, views.data(), (uint32_t)views.size(), rgb8.data(), &st);
    if (rc == RT_ERR_UNSUPPORTED && !accumulate && !camera_kind) {
        std::vector<float> fb(n_out * view_pixels * 3, 0.0f);
        rc = views.empty() ? rt_render(scene, &p, fb.data(), &st) : rt_render_views(scene, &p, views.data(), (uint32_t)views.size(), fb.data(), &st);
        if (rc == RT_OK)
            rt_tonemap_rgb8(fb.data(), n_out * view_pixels, rgb8.data());
    }
    rt_destroy(scene);
    rt_loaded_free(loaded);
    if (rc != RT_OK)
        return die("rt_render");
    if (views.empty()) {
        if (rt_write_ppm(argv[5], width, height, rgb8.data()) != RT_OK)
            return die("write");
    } else {
        const std::filesystem::path out(argv[5]);
        for (size_t i = 0; i < n_out; ++i) {
            std::filesystem::path name = out.parent_path() / (out.stem().string() + "_" + std::to_string(i) + out.extension().string());
            if (rt_write_ppm(name.string().c_str(), width, height, rgb8.data() + i * view_pixels * 3) != RT_OK)
                return die("write");
        }
    }
    if (light_groups) {
        const std::filesystem::path out(argv[5]);
        for (uint32_t g = 0; g < n_groups; ++g) {
            std::filesystem::path name = out.parent_path() / (out.stem().string() + "_group_" + std::to_string(g) + out.extension().string());
            if (rt_write_ppm(name.string().c_str(), width, height, group_rgb8.data() + (size_t)g * view_pixels * 3) != RT_OK)
                return die("RT_LIGHT_GROUPS");
        }
    }
    if (aov) {
        auto quantise = [&](const std::vector<float> &v, float scale, float bias) {
            std::vector<uint8_t> q(v.size());
            for (size_t i = 0; i < v.size(); ++i) {
                const float x = v[i] * scale + bias;
                q[i] = (uint8_t)(std::min(std::max(x, 0.0f), 1.0f) * 255.0f + 0.5f);
            }
            return q;
        };
        const std::string prefix(aov);
        if (rt_write_ppm((prefix + "_albedo.ppm").c_str(), width, height, quantise(aov_albedo, 1.0f, 0.0f).data()) != RT_OK ||
            rt_write_ppm((prefix + "_normal.ppm").c_str(), width, height, quantise(aov_normal, 0.5f, 0.5f).data()) != RT_OK)
            return die("RT_AOV");
        FILE *f = std::fopen((prefix + "_depth.pfm").c_str(), "wb");
        if (!f) {
            std::cerr << "RT_AOV: cannot write " << prefix << "_depth.pfm" << std::endl;
            return EXIT_FAILURE;
        }
        std::fprintf(f, "Pf\n%u %u\n-1.0\n", width, height); // negative scale: little-endian
        for (unsigned y = height; y-- > 0;)
            std::fwrite(aov_depth.data() + (size_t)y * width, sizeof(float), width, f);
        std::fclose(f);
    }
    if (adaptive) {
        if (const char *map_path = std::getenv("RT_SPP_MAP")) { // binary 16-bit PGM, big-endian, counts clamped to 65535
            FILE *f = std::fopen(map_path, "wb");
            if (!f)
                return die("RT_SPP_MAP");
            std::fprintf(f, "P5\n%u %u\n65535\n", width, height);
            for (uint32_t c : spp_map) {
                const uint32_t v = std::min(c, 65535u);
                std::fputc((int)(v >> 8), f);
                std::fputc((int)(v & 255u), f);
            }
            std::fclose(f);
        }
        if (verbose) {
            double total = 0;
            for (uint32_t c : spp_map)
                total += c;
            std::fprintf(stderr, "adaptive: rounds=%u mean_spp=%.3f\n", rounds, spp_map.empty() ? 0.0 : total / (double)spp_map.size());
        }
    }
    if (verbose)
        std::fprintf(stderr, "samples=%llu kernel_ms=%.3f Msamples/s=%.3f\n", (unsigned long long)st.samples, st.kernel_ms,
                     st.kernel_ms > 0 ? st.samples / st.kernel_ms / 1e3 : 0.0);
    return EXIT_SUCCESS;
}
