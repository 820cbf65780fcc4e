// rt_tex_views.h — how a group of equally sized textures is laid out in the texel pool (host, header only): the ONE place that decides
// a view's layout. rt_create (rt_scene.cpp) calls build_texture_views for every group; the kernels read what it wrote through DevTexture
// (rt_dev_surface.h: tex_tiled, tex_sample, tex_sample_set). Three layouts (rt_device_types.h DevTexture):
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
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rt_device_types.h"

namespace rt {

constexpr size_t TEX_FOOT_CAP_DWORDS = (size_t)1 << 29; // 2 GiB of footprint records per scene

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

} // namespace rt
