// rt_accum_layers.cpp — the optional layers of an accumulator (rt_accum_impl.h): first-hit features with the denoiser, id mattes, light
// groups, each with its attach / read / resolve entry points. The passes that fill them are rt_accum_host.cpp's; the kernels are
// rt_wavefront.hip (wf_features, wf_ids, wf_group_tags), rt_wf_stages.h (the folds and resolves), rt_accum.hip and rt_denoise.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rt_accum_impl.h"

using rt::AccumNeed;

// ---- the attach protocol of a layer that arrives after creation (`noun`: "ids", "light groups")
static int attach_aligned(const void *table, bool device_table, const char *fn) {
    if (device_table && (reinterpret_cast<uintptr_t>(table) & 3u))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the device table must be 4-byte aligned");
    return RT_OK;
}
static int attach_in_time(const rt_accum *acc, bool has, const char *noun, const char *fn) {
    if (has)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the accumulator already has " + noun);
    if (acc->has_samples)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": the accumulator already holds samples; attach " + noun + " before the first render");
    return RT_OK;
}
// The layer's arrays in the accumulator's arena: the sums (zeroed), then the table (null: none), a copy of `src`; the caller publishes its
// record only when all of this is done. A failure leaves what was allocated with the arena, unused, until rt_accum_destroy. `src` may be a
// local of the caller: nothing is in flight at the return.
struct AttachArray {
    void **ptr;
    size_t bytes;
};
static int attach_arrays(rt_accum *acc, const char *fn, std::initializer_list<AttachArray> sums, AttachArray table, const void *src, bool device_table) {
    rt_scene *s = acc->scene;
    for (const AttachArray &a : sums)
        if (int rc = rt::accum_alloc(acc, a.bytes, a.ptr, fn); rc != RT_OK)
            return rc;
    if (table.ptr)
        if (int rc = rt::accum_alloc(acc, table.bytes, table.ptr, fn); rc != RT_OK)
            return rc;
    return rt::queue_and_wait(s->stream, [&]() -> int {
        for (const AttachArray &a : sums)
            HIP_TRY(hipMemsetAsync(*a.ptr, 0, a.bytes, s->stream)); // +0.0
        if (table.ptr && table.bytes)
            HIP_TRY(hipMemcpyAsync(*table.ptr, src, table.bytes, device_table ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s->stream));
        return RT_OK;
    });
}

// ---- first-hit features and the denoiser (rt_abi.h RT_ACCUM_FEATURES, rt_accum_denoise)
extern "C" int rt_accum_read_features(rt_accum *acc, float *albedo_sum, float *normal_sum, float *depth_sum, uint32_t *hits) {
    if (int rc = rt::accum_entry(acc, "rt_accum_read_features", AccumNeed::FEATURES); rc != RT_OK)
        return rc;
    const WfFeat &F = *acc->features;
    const size_t n = (size_t)acc->width * acc->height;
    return rt::read_back(acc, {{albedo_sum, F.albedo_sum, 12 * n}, {normal_sum, F.normal_sum, 12 * n}, {depth_sum, F.depth_sum, 4 * n}, {hits, F.hits, 4 * n}});
}

extern "C" int rt_accum_resolve_features(rt_accum *acc, uint32_t flags, float *albedo, float *normal, float *depth) {
    if (int rc = rt::accum_entry(acc, "rt_accum_resolve_features", AccumNeed::FEATURES); rc != RT_OK)
        return rc;
    if (rt::other_flags(flags))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_resolve_features: flags other than RT_FLAG_DEVICE_FB");
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = (size_t)acc->width * acc->height;
    rt::CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    float *d_a, *d_n, *d_z; // on a host call all three are computed; a null destination is not copied
    io.out(&d_a, albedo, 12 * n);
    io.out(&d_n, normal, 12 * n);
    io.out(&d_z, depth, 4 * n);
    return io.run([&]() -> int {
        HIP_TRY(rt::launch_accum_feature_means(acc->R, *acc->features, d_a, d_n, d_z, s->stream));
        return RT_OK;
    });
}

// a read of one buffer that must be there: the second test of the denoiser's and the light groups' entry points
static int accum_entry_out(const rt_accum *acc, const char *fn, AccumNeed need, const void *buffer, uint32_t flags) {
    if (int rc = rt::accum_entry(acc, fn, need); rc != RT_OK)
        return rc;
    if (!buffer || rt::other_flags(flags))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null buffer or flags other than RT_FLAG_DEVICE_FB");
    return RT_OK;
}

// the defaults of rt_denoise: chosen by the sweep recorded in profiles/denoise_quality.txt
static int denoise_options(const rt_denoise *opt, const char *fn, rt::DenoiseOpt *O) {
    const rt_denoise zero{};
    const rt_denoise &o = opt ? *opt : zero;
    for (uint32_t r : o.reserved)
        if (r != 0)
            return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": reserved fields must be 0");
    if (o.iterations > 8u || o.normal_sharpness > 8u || (o.flags & ~(uint32_t)RT_DENOISE_NO_DEMODULATE))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": iterations and normal_sharpness are at most 8; unknown rt_denoise.flags bit");
    if (!(o.sigma_color >= 0.0f) || std::isinf(o.sigma_color) || !(o.sigma_depth >= 0.0f) || std::isinf(o.sigma_depth))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": sigma_color and sigma_depth must be finite and >= 0");
    O->iterations = o.iterations ? o.iterations : 5u;
    O->sigma_color = o.sigma_color != 0.0f ? o.sigma_color : 8.0f;
    O->sigma_depth = o.sigma_depth != 0.0f ? o.sigma_depth : 0.5f;
    O->sharpness = o.normal_sharpness ? o.normal_sharpness : 3u;
    O->demodulate = (o.flags & RT_DENOISE_NO_DEMODULATE) ? 0u : 1u;
    return RT_OK;
}

static int denoise_buffers(rt_accum *acc, const char *fn) {
    if (acc->D.guide)
        return RT_OK;
    const size_t n = (size_t)acc->width * acc->height;
    int rc;
    if ((rc = rt::accum_alloc(acc, 16 * n, &acc->D.sig[0], fn)) != RT_OK || (rc = rt::accum_alloc(acc, 16 * n, &acc->D.sig[1], fn)) != RT_OK ||
        (rc = rt::accum_alloc(acc, 16 * n, &acc->D.den, fn)) != RT_OK)
        return rc;
    return rt::accum_alloc(acc, 32 * n, &acc->D.guide, fn); // last: its pointer says the workspace is complete
}

template <class Out> static int denoise(rt_accum *acc, const rt_denoise *opt, uint32_t flags, Out *out, const char *fn) {
    rt::DenoiseOpt O{};
    int rc;
    if ((rc = accum_entry_out(acc, fn, AccumNeed::FEATURES, out, flags)) != RT_OK || (rc = denoise_options(opt, fn, &O)) != RT_OK)
        return rc;
    HIP_TRY(hipSetDevice(acc->scene->device)); // the workspace is allocated before the call's arrays are declared
    if ((rc = denoise_buffers(acc, fn)) != RT_OK)
        return rc;
    return rt::accum_image(acc, flags, out, [&](float *d_fb) { return rt::launch_denoise(acc->R, *acc->features, acc->D, O, d_fb, acc->scene->stream); });
}
extern "C" int rt_accum_denoise(rt_accum *acc, const rt_denoise *opt, uint32_t flags, float *fb_rgb) { return denoise(acc, opt, flags, fb_rgb, "rt_accum_denoise"); }
extern "C" int rt_accum_denoise_rgb8(rt_accum *acc, const rt_denoise *opt, uint32_t flags, uint8_t *rgb8) {
    return denoise(acc, opt, flags, rgb8, "rt_accum_denoise_rgb8");
}

// ---- id mattes (rt_abi.h rt_accum_attach_ids: the rule; the kernels: rt_wavefront.hip wf_ids / wf_resolve_ids, rt_accum.hip)
extern "C" int rt_accum_attach_ids(rt_accum *acc, const rt_id_desc *desc) {
    const char *fn = "rt_accum_attach_ids";
    if (!acc || !desc)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: null argument");
    rt_scene *s = acc->scene;
    const bool user = desc->kind == RT_ID_USER, device_table = (desc->flags & RT_FLAG_DEVICE_FB) != 0;
    if (desc->kind > (uint32_t)RT_ID_USER)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: unknown kind " + std::to_string(desc->kind));
    if (desc->slots > RT_ID_MAX_SLOTS)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: slots must be 0 (= 4) or 1..16");
    if (desc->reserved[0] != 0 || desc->reserved[1] != 0 || rt::other_flags(desc->flags))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: reserved fields must be 0; flags other than RT_FLAG_DEVICE_FB");
    const uint32_t n_table = s->dev.n_triangles + s->dev.n_prims;
    if (user && (!desc->table || desc->n_table != n_table))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: RT_ID_USER needs a table of n_triangles + n_primitives = " + std::to_string(n_table) + " ids");
    if (!user && (desc->table || desc->n_table != 0))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_attach_ids: only RT_ID_USER takes a table");
    int rc;
    if ((rc = attach_aligned(desc->table, user && device_table, fn)) != RT_OK || (rc = attach_in_time(acc, acc->ids.has_value(), "ids", fn)) != RT_OK)
        return rc;
    HIP_TRY(hipSetDevice(s->device));
    WfIds I{};
    I.kind = desc->kind;
    I.k = desc->slots ? desc->slots : 4u;
    I.pixels = acc->width * acc->height;
    const size_t n = I.pixels, words = n * I.k;
    void *table = nullptr;
    if ((rc = attach_arrays(acc, fn, {{(void **)&I.slot_id, 4 * words}, {(void **)&I.slot_count, 4 * words}, {(void **)&I.other, 4 * n}},
                            {user ? &table : nullptr, 4 * (size_t)n_table}, desc->table, device_table)) != RT_OK)
        return rc;
    I.table = static_cast<uint32_t *>(table);
    acc->ids = I;
    return RT_OK;
}

extern "C" int rt_accum_read_ids(rt_accum *acc, uint32_t *ids, uint32_t *counts, uint32_t *other) {
    if (int rc = rt::accum_entry(acc, "rt_accum_read_ids", AccumNeed::IDS); rc != RT_OK)
        return rc;
    const WfIds &I = *acc->ids;
    const size_t n = I.pixels, K = I.k;
    std::vector<uint32_t> slot_major; // the device keeps slot j of pixel p at j * pixels + p
    for (auto [dst, src] : {std::pair{ids, I.slot_id}, std::pair{counts, I.slot_count}}) {
        if (!dst)
            continue;
        slot_major.resize(n * K);
        if (int rc = rt::read_back(acc, {{slot_major.data(), src, 4 * n * K}}); rc != RT_OK)
            return rc;
        for (size_t p = 0; p < n; ++p)
            for (size_t j = 0; j < K; ++j)
                dst[p * K + j] = slot_major[j * n + p];
    }
    return rt::read_back(acc, {{other, I.other, 4 * n}});
}

extern "C" int rt_accum_resolve_labels(rt_accum *acc, uint32_t flags, uint32_t *label, float *coverage) {
    if (int rc = rt::accum_entry(acc, "rt_accum_resolve_labels", AccumNeed::IDS); rc != RT_OK)
        return rc;
    if (rt::other_flags(flags))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_resolve_labels: flags other than RT_FLAG_DEVICE_FB");
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    rt::CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    uint32_t *d_label;
    float *d_cov;
    io.out(&d_label, label, 4 * (size_t)acc->ids->pixels);
    io.out(&d_cov, coverage, 4 * (size_t)acc->ids->pixels);
    return io.run([&]() -> int {
        HIP_TRY(rt::launch_accum_labels(acc->R, *acc->ids, d_label, d_cov, s->stream));
        return RT_OK;
    });
}

extern "C" int rt_accum_resolve_matte(rt_accum *acc, uint32_t flags, const uint32_t *ids, uint32_t n_ids, float *matte) {
    if (int rc = rt::accum_entry(acc, "rt_accum_resolve_matte", AccumNeed::IDS); rc != RT_OK)
        return rc;
    if (!ids || !matte || n_ids == 0 || n_ids > 4096u || rt::other_flags(flags))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_resolve_matte: null ids or matte, n_ids outside 1..4096, or flags other than RT_FLAG_DEVICE_FB");
    rt_scene *s = acc->scene;
    HIP_TRY(hipSetDevice(s->device));
    std::vector<uint32_t> set(ids, ids + n_ids); // sorted, each id once: the kernel's binary search
    std::sort(set.begin(), set.end());
    set.erase(std::unique(set.begin(), set.end()), set.end());
    HIP_TRY(acc->matte_set.reserve(set.size()));
    rt::CallIo io(s->stream, s->staging, (flags & RT_FLAG_DEVICE_FB) != 0);
    float *d_matte;
    io.out(&d_matte, matte, 4 * (size_t)acc->ids->pixels);
    return io.run([&]() -> int { // `set` is a local: nothing of this may be in flight when it dies
        HIP_TRY(hipMemcpyAsync(acc->matte_set.get(), set.data(), 4 * set.size(), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(rt::launch_accum_matte(acc->R, *acc->ids, acc->matte_set.get(), (uint32_t)set.size(), d_matte, s->stream));
        return RT_OK;
    });
}

// ---- light groups (rt_abi.h rt_accum_attach_light_groups: the rule; the kernels: rt_wavefront.hip wf_group_tags, rt_wf_stages.h wf_fold_groups /
// wf_resolve_groups, rt_accum.hip)
extern "C" int rt_accum_attach_light_groups(rt_accum *acc, const rt_light_group_desc *desc) {
    const char *fn = "rt_accum_attach_light_groups";
    if (!acc || !desc)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null argument");
    rt_scene *s = acc->scene;
    const uint32_t G = desc->n_groups, n_mats = (uint32_t)s->prep->mats.size();
    const bool device_table = (desc->flags & RT_FLAG_DEVICE_FB) != 0;
    auto in_range = [G](uint32_t g) { return g < G || g == RT_LIGHT_GROUP_NONE; };
    if (G == 0 || G > RT_LIGHT_GROUP_MAX)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": n_groups must be 1.." + std::to_string(RT_LIGHT_GROUP_MAX));
    if (desc->reserved[0] != 0 || desc->reserved[1] != 0 || rt::other_flags(desc->flags))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": reserved fields must be 0; flags other than RT_FLAG_DEVICE_FB");
    if (!desc->material_group || desc->n_materials != n_mats)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": material_group must hold the scene's " + std::to_string(n_mats) + " materials");
    if (int rc = attach_aligned(desc->material_group, device_table, fn); rc != RT_OK)
        return rc;
    if (!in_range(desc->background_group))
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": background_group must be below n_groups, or RT_LIGHT_GROUP_NONE");
    if (int rc = attach_in_time(acc, acc->groups.has_value(), "light groups", fn); rc != RT_OK)
        return rc;
    HIP_TRY(hipSetDevice(s->device));
    std::vector<uint32_t> words(n_mats); // the entries are checked on the host, wherever the table lives
    if (device_table) {
        if (int rc = rt::queue_and_wait(s->stream, [&]() -> int {
                HIP_TRY(hipMemcpyAsync(words.data(), desc->material_group, 4 * (size_t)n_mats, hipMemcpyDeviceToHost, s->stream));
                return RT_OK;
            });
            rc != RT_OK)
            return rc;
    } else {
        std::copy(desc->material_group, desc->material_group + n_mats, words.begin());
    }
    std::vector<uint8_t> bytes(n_mats);
    for (uint32_t m = 0; m < n_mats; ++m) {
        if (!in_range(words[m]))
            return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": material_group[" + std::to_string(m) + "] is neither below n_groups nor RT_LIGHT_GROUP_NONE");
        bytes[m] = words[m] == RT_LIGHT_GROUP_NONE ? (uint8_t)WF_GROUP_NONE : (uint8_t)words[m];
    }
    WfGroups W{};
    W.n_groups = G;
    W.background = desc->background_group == RT_LIGHT_GROUP_NONE ? WF_GROUP_NONE : desc->background_group;
    W.pixels = acc->width * acc->height;
    void *table = nullptr; // the checked bytes go up from the host, wherever the words came from
    if (int rc = attach_arrays(acc, fn, {{(void **)&W.sum, 12 * (size_t)G * W.pixels}}, {&table, n_mats}, bytes.data(), false); rc != RT_OK)
        return rc;
    W.material_group = static_cast<uint8_t *>(table);
    acc->groups = W;
    return RT_OK;
}

extern "C" int rt_accum_read_light_groups(rt_accum *acc, float *group_sums) {
    if (int rc = accum_entry_out(acc, "rt_accum_read_light_groups", AccumNeed::GROUPS, group_sums, 0u); rc != RT_OK)
        return rc;
    return rt::read_back(acc, {{group_sums, acc->groups->sum, 12 * (size_t)acc->groups->n_groups * acc->groups->pixels}});
}

extern "C" int rt_accum_resolve_light_group(rt_accum *acc, uint32_t group, uint32_t flags, float *fb_rgb) {
    if (int rc = accum_entry_out(acc, "rt_accum_resolve_light_group", AccumNeed::GROUPS, fb_rgb, flags); rc != RT_OK)
        return rc;
    if (group >= acc->groups->n_groups)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_accum_resolve_light_group: group " + std::to_string(group) + " of " + std::to_string(acc->groups->n_groups));
    return rt::accum_image(acc, flags, fb_rgb, [&](float *d_fb) { return rt::launch_accum_light_group(acc->R, *acc->groups, group, d_fb, acc->scene->stream); });
}

// the G x 3 weights of a mix travel as the kernel argument `w`
template <class Out> static int light_mix(rt_accum *acc, const float *weights, uint32_t flags, Out *out, const char *fn) {
    if (int rc = accum_entry_out(acc, fn, AccumNeed::GROUPS, out, flags); rc != RT_OK)
        return rc;
    if (!weights)
        return rt::fail(RT_ERR_INVALID_ARG, std::string(fn) + ": null weights");
    rt::LightMixWeights w{};
    std::memcpy(w.w, weights, 12 * (size_t)acc->groups->n_groups);
    return rt::accum_image(acc, flags, out, [&](float *d_fb) { return rt::launch_accum_light_mix(acc->R, *acc->groups, w, d_fb, acc->scene->stream); });
}
extern "C" int rt_accum_resolve_light_mix(rt_accum *acc, const float *weights, uint32_t flags, float *fb_rgb) {
    return light_mix(acc, weights, flags, fb_rgb, "rt_accum_resolve_light_mix");
}
extern "C" int rt_accum_resolve_light_mix_rgb8(rt_accum *acc, const float *weights, uint32_t flags, uint8_t *rgb8) {
    return light_mix(acc, weights, flags, rgb8, "rt_accum_resolve_light_mix_rgb8");
}
