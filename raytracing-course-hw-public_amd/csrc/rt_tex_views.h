// rt_tex_views.h — the texel pool of a scene (host, header only): the ONE place that decides which of a material's textures form a view
// (assign_texture_views, which rt_create calls once: rt_scene_prepare.cpp) and how a view is laid out (build_texture_views, for every group).
// The kernels read what they wrote through DevTexture (rt_dev_surface.h: tex_tiled, tex_sample, tex_sample_set). Three layouts
// (rt_device_types.h DevTexture):
//   stride 1   a texture on its own: texels in tiles of 8 x 4 (128 B);
//   stride 4   an interleaved set: record (x, y) = the members' texels at (x, y), 16 B, in tiles of 4 x 2 records (128 B);
//   stride 16  a FOOTPRINT set: record (x0, y0) = {q00, q01, q10, q11}, the four 16-byte set records a bilinear lookup with base texel
//              (x0, y0) reads (Texture::sample's neighbours, geometry.h:545-563: x1 = x0 + 1 wrapping to 0, y1 alike; a 1 x 1 texture's
//              four are the same texel), 64 B and 64-byte aligned, in tiles of 4 x 2 records. A lookup is one address and one line where the
//              interleaved set's 2 x 2 footprint straddles a tile edge for 7 lookups of 8 (1.875 lines on average). q00 of record (x, y) IS
//              the set record of (x, y), so whatever reads texel (x, y) of a member (tex_sample, the out-of-range path of TexFoot::fetch)
//              reads it at tiled index * stride as in the other two layouts.
// Footprint sets take 4 x the memory of interleaved ones, so they are built only while the scene's footprint records stay below a cap
// (TEX_FOOT_CAP_DWORDS, DESIGN.md "Data layout in HBM"); a group beyond it, and every group of a scene created with RT_BUILD_TEX_TILED,
// is an interleaved set.
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rt_device_types.h"

namespace rt {

constexpr size_t TEX_FOOT_CAP_DWORDS = (size_t)1 << 29;   // 2 GiB of footprint records per scene
constexpr size_t TEX_SET_BUDGET_DWORDS = (size_t)1 << 30; // 4 GiB of pool, beyond which no further set is interleaved

// tiled index of record (x, y) of a view: rt_dev_surface.h tex_tiled, for the host
inline size_t tex_tiled_index(const DevTexture &T, uint32_t x, uint32_t y) {
    const size_t tile = (size_t)(y >> T.th_log) * T.tiles_x + (x >> T.tw_log);
    const size_t within = ((y & ((1u << T.th_log) - 1u)) << T.tw_log) | (x & ((1u << T.tw_log) - 1u));
    return (tile << (T.tw_log + T.th_log)) + within;
}
// records (tile padding included) of a w x h view with these tiles
inline size_t tex_view_records(uint32_t w, uint32_t h, uint32_t tw_log, uint32_t th_log) {
    const size_t tiles_x = ((size_t)w + (1u << tw_log) - 1) >> tw_log, tiles_y = ((size_t)h + (1u << th_log) - 1) >> th_log;
    return tiles_x * tiles_y << (tw_log + th_log);
}

// Appends the views of one group to the pool. members[k]: the w x h RGBA8 texels of the texture in record dword k, row-major, or null for an
// unused slot; n_members is 1 (a texture on its own) or 4 (a set). `foot_dwords` is the scene's running total of footprint records, `foot_cap`
// its cap, `force_tiled` the scene's RT_BUILD_TEX_TILED. view_of_member[k] = the new view's index in texs, or -1. The region appended is
// [aligned base, base + records * stride): 128-byte aligned, tile padding zero.
inline void build_texture_views(std::vector<uint32_t> &pool, std::vector<DevTexture> &texs, const uint32_t *const *members, uint32_t n_members, uint32_t w, uint32_t h,
                                bool force_tiled, size_t foot_cap, size_t &foot_dwords, int32_t *view_of_member) {
    const bool set = n_members > 1;
    const uint32_t tw_log = set ? 2u : 3u, th_log = set ? 1u : 2u; // 8 x 4 texels, or 4 x 2 records
    const size_t records = tex_view_records(w, h, tw_log, th_log);
    const bool foot = set && !force_tiled && foot_dwords + records * RT_TEX_FOOT_STRIDE <= foot_cap;
    const uint32_t stride = !set ? 1u : foot ? RT_TEX_FOOT_STRIDE : 4u;
    const size_t base = (pool.size() + 31) & ~size_t(31); // 128-B aligned tiles
    pool.resize(base + records * stride, 0u);
    if (foot)
        foot_dwords += records * stride;
    DevTexture T{w, h, (uint32_t)base, w * h, stride, (uint32_t)((w + (1u << tw_log) - 1) >> tw_log), tw_log, th_log};
    for (uint32_t k = 0; k < n_members; ++k) {
        view_of_member[k] = -1;
        const uint32_t *src = members[k];
        if (!src)
            continue;
        uint32_t *dst = pool.data() + base + k;
        for (uint32_t y = 0; y < h; ++y) {
            const uint32_t *row0 = src + (size_t)y * w, *row1 = src + (size_t)(y == h - 1 ? 0 : y + 1) * w;
            for (uint32_t x = 0; x < w; ++x) {
                uint32_t *rec = dst + tex_tiled_index(T, x, y) * stride;
                rec[0] = row0[x];
                if (foot) { // q01 = (x0, y1), q10 = (x1, y0), q11 = (x1, y1)
                    const uint32_t x1 = x == w - 1 ? 0 : x + 1;
                    rec[4] = row1[x];
                    rec[8] = row0[x1];
                    rec[12] = row1[x1];
                }
            }
        }
        view_of_member[k] = (int32_t)texs.size();
        DevTexture V = T;
        V.offset = (uint32_t)(base + k);
        texs.push_back(V);
    }
}

using TexSlots = std::array<int32_t, 4>; // per slot (colour, emissive, metallic-roughness, normal) a texture or a view, -1 = none
inline TexSlots tex_slots(const DevMaterial &m) { return {m.color_tex, m.emissive_tex, m.mr_tex, m.normal_tex}; }

// One interleaved set serves ALL of a material's lookups? Then wf_shade computes the texel addresses once and reads the four members of a
// record with one 16-byte load (tex_sample_set), or all four records of the lookup from one line when the set holds footprint records. A
// member's record dword is its slot index.
inline void find_tex_set(const std::vector<DevTexture> &texs, const TexSlots &view, DevMaterial &m) {
    m.tex_set = -1;
    m.tex_set_info = 0;
    uint32_t present = 0;
    int first = -1;
    bool one_set = true;
    for (int a = 0; a < 4; ++a) {
        if (view[a] < 0)
            continue;
        present |= 1u << a;
        const DevTexture &t = texs[view[a]];
        if (t.stride < 4u) // neither an interleaved nor a footprint set
            one_set = false;
        else if (first < 0)
            first = a;
        else if (t.offset - (uint32_t)a != texs[view[first]].offset - (uint32_t)first)
            one_set = false; // another set's records
    }
    if (one_set && first >= 0) {
        m.tex_set = view[first];
        m.tex_set_info = present | ((uint32_t)first << 4);
    }
}

// Of a material's textures the largest group that shares a size (> 1x1; the earlier slot's group wins a tie), or nothing for a group of one.
inline TexSlots largest_tex_group(const rt_texture_desc *textures, const TexSlots &ids) {
    TexSlots group = {-1, -1, -1, -1};
    int best_n = 1;
    for (int a = 0; a < 4; ++a) {
        if (ids[a] < 0 || textures[ids[a]].width * textures[ids[a]].height == 1)
            continue;
        TexSlots g = {-1, -1, -1, -1};
        int n = 0;
        for (int b = 0; b < 4; ++b)
            if (ids[b] >= 0 && textures[ids[b]].width == textures[ids[a]].width && textures[ids[b]].height == textures[ids[a]].height) {
                g[b] = ids[b];
                ++n;
            }
        if (n > best_n) {
            best_n = n;
            group = g;
        }
    }
    return group;
}

// The views of a scene: tiled storage, and the textures one material samples together at equal size interleaved record by record. A material
// slot refers to a VIEW: on entry the four slots of a record of `mats` name textures, on return views, and tex_set / tex_set_info are set.
// A material's largest group is interleaved while the pool is below `set_budget` dwords, its other textures stand alone; equal slot tuples
// share their views. Pool order (offsets and view ids follow from it): per material in turn its set, then the stand-alone views of its other
// slots, each built at first need; the stand-alone view of bg_texture (Scene::bg scene.h:81: sampled on its own) last.
inline void assign_texture_views(const rt_texture_desc *textures, uint32_t n_textures, int32_t bg_texture, bool force_tiled, size_t foot_cap, size_t set_budget,
                                 std::vector<DevMaterial> &mats, std::vector<uint32_t> &pool, std::vector<DevTexture> &texs, int32_t &bg_view) {
    size_t foot_dwords = 0; // footprint records of this scene so far, against foot_cap
    auto store = [&](const TexSlots &members, uint32_t n_members, int32_t *views) { // members: equal size, one per record dword
        const rt_texture_desc *any = nullptr;
        const uint32_t *src[4] = {nullptr, nullptr, nullptr, nullptr};
        for (uint32_t k = 0; k < n_members; ++k)
            if (members[k] >= 0)
                src[k] = reinterpret_cast<const uint32_t *>((any = &textures[members[k]])->rgba8);
        build_texture_views(pool, texs, src, n_members, any->width, any->height, force_tiled, foot_cap, foot_dwords, views);
    };
    std::vector<int32_t> alone(n_textures, -1); // stand-alone view of texture i
    auto alone_view = [&](int32_t t) {
        if (alone[t] < 0)
            store({t, -1, -1, -1}, 1u, &alone[t]);
        return alone[t];
    };
    std::vector<TexSlots> slots(mats.size()), views(mats.size(), TexSlots{-1, -1, -1, -1});
    for (size_t i = 0; i < mats.size(); ++i) {
        DevMaterial &m = mats[i];
        const TexSlots ids = slots[i] = tex_slots(m);
        TexSlots &view = views[i];
        if (const auto same = std::find(slots.begin(), slots.begin() + i, ids); same != slots.begin() + i) {
            view = views[same - slots.begin()];
        } else {
            if (const TexSlots group = largest_tex_group(textures, ids); group != view && pool.size() < set_budget)
                store(group, 4u, view.data());
            for (int a = 0; a < 4; ++a)
                if (ids[a] >= 0 && view[a] < 0)
                    view[a] = alone_view(ids[a]);
        }
        m.color_tex = view[0], m.emissive_tex = view[1], m.mr_tex = view[2], m.normal_tex = view[3];
        find_tex_set(texs, view, m);
    }
    bg_view = bg_texture >= 0 ? alone_view(bg_texture) : -1;
}

} // namespace rt
