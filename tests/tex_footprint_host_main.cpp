// tests/tex_footprint_host_main.cpp — csrc/rt_tex_views.h on the CPU, stand-alone (tests/test_tex_footprint_host.py builds it with the address
// and undefined-behaviour sanitizers). For every size: each base texel's footprint record equals the four records that a plain restatement of
// TexFoot's neighbour rule (rt_dev_surface.h; Texture::sample, geometry.h:545-563) reads from the interleaved tiled layout of the same
// textures; the pool region is exactly covered; views over the cap, and every view of a forced-tiled build, fall back to tiles.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_tex_views.h"

static unsigned long long g_checks = 0;
#define CHECK(c)                                                            \
    do {                                                                    \
        ++g_checks;                                                         \
        if (!(c)) {                                                         \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

// the tiled index written out once more, on its own: tiles of 2^tw x 2^th records, row-major tiles, row-major inside a tile
static size_t tiled_plain(uint32_t w, uint32_t tw, uint32_t th, uint32_t x, uint32_t y) {
    const uint32_t TW = 1u << tw, TH = 1u << th;
    const size_t tiles_x = (w + TW - 1) / TW;
    return ((size_t)(y / TH) * tiles_x + x / TW) * TW * TH + (size_t)(y % TH) * TW + x % TW;
}
static size_t records_plain(uint32_t w, uint32_t h, uint32_t tw, uint32_t th) {
    const uint32_t TW = 1u << tw, TH = 1u << th;
    return (size_t)((w + TW - 1) / TW) * ((h + TH - 1) / TH) * TW * TH;
}
// texel (x, y) of member k of texture group g: never zero, different everywhere
static uint32_t texel(uint32_t g, uint32_t k, uint32_t w, uint32_t x, uint32_t y) { return 0x80000000u | (g << 24) | (k << 20) | (y * w + x); }

struct Built {
    std::vector<uint32_t> pool;
    std::vector<DevTexture> texs;
    int32_t views[4] = {-1, -1, -1, -1};
    size_t foot = 0, before = 0;
};
static Built build(uint32_t g, uint32_t w, uint32_t h, unsigned present, bool force_tiled, size_t cap, size_t foot_before, size_t lead) {
    std::vector<std::vector<uint32_t>> src(4);
    const uint32_t *members[4] = {nullptr, nullptr, nullptr, nullptr};
    for (uint32_t k = 0; k < 4; ++k)
        if (present & (1u << k)) {
            src[k].resize((size_t)w * h);
            for (uint32_t y = 0; y < h; ++y)
                for (uint32_t x = 0; x < w; ++x)
                    src[k][(size_t)y * w + x] = texel(g, k, w, x, y);
            members[k] = src[k].data();
        }
    Built b;
    b.pool.assign(lead, 0xDEADBEEFu); // what earlier views left in the pool: the new region starts at the next 128-byte boundary
    b.before = lead;
    b.foot = foot_before;
    rt::build_texture_views(b.pool, b.texs, members, 4u, w, h, force_tiled, cap, b.foot, b.views);
    return b;
}

static void check_size(uint32_t g, uint32_t w, uint32_t h, unsigned present) {
    const size_t recs = records_plain(w, h, 2, 1), lead = 5 + g; // an unaligned lead-in
    const size_t base = (lead + 31) / 32 * 32;
    const Built T = build(g, w, h, present, true, rt::TEX_FOOT_CAP_DWORDS, 0, lead);   // interleaved 16-byte records in 4 x 2 tiles
    const Built F = build(g, w, h, present, false, rt::TEX_FOOT_CAP_DWORDS, 7, lead);  // footprint records
    CHECK(T.pool.size() == base + recs * 4 && T.foot == 0);
    CHECK(F.pool.size() == base + recs * 16 && F.foot == 7 + recs * 16);
    CHECK(base % 16 == 0); // 64-byte aligned records
    for (size_t i = 0; i < lead; ++i)
        CHECK(T.pool[i] == 0xDEADBEEFu && F.pool[i] == 0xDEADBEEFu);
    for (size_t i = lead; i < base; ++i)
        CHECK(T.pool[i] == 0u && F.pool[i] == 0u);
    unsigned n_views = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        if (!(present & (1u << k))) {
            CHECK(T.views[k] == -1 && F.views[k] == -1);
            continue;
        }
        CHECK(T.views[k] == (int32_t)n_views && F.views[k] == (int32_t)n_views);
        ++n_views;
        const DevTexture &t = T.texs[T.views[k]], &f = F.texs[F.views[k]];
        CHECK(t.width == w && t.height == h && t.count == w * h && t.offset == base + k && t.stride == 4u && t.tw_log == 2u && t.th_log == 1u && t.tiles_x == (w + 3) / 4);
        CHECK(f.width == w && f.height == h && f.count == w * h && f.offset == base + k && f.stride == RT_TEX_FOOT_STRIDE && f.tw_log == 2u && f.th_log == 1u && f.tiles_x == (w + 3) / 4);
        // the host's index function is the plain one
        for (uint32_t y = 0; y < h; ++y)
            for (uint32_t x = 0; x < w; ++x)
                CHECK(rt::tex_tiled_index(f, x, y) == tiled_plain(w, 2, 1, x, y));
    }
    CHECK(T.texs.size() == n_views && F.texs.size() == n_views);
    // the tiled layout holds the textures; every footprint record is the four tiled records of TexFoot's neighbours
    std::vector<uint8_t> covered(recs, 0);
    for (uint32_t y0 = 0; y0 < h; ++y0)
        for (uint32_t x0 = 0; x0 < w; ++x0) {
            const uint32_t x1 = x0 == w - 1 ? 0 : x0 + 1, y1 = y0 == h - 1 ? 0 : y0 + 1; // mod_inc
            const size_t r = tiled_plain(w, 2, 1, x0, y0);
            CHECK(r < recs && !covered[r]);
            covered[r] = 1;
            const uint32_t *rec = F.pool.data() + base + r * 16;
            const uint32_t nx[4] = {x0, x0, x1, x1}, ny[4] = {y0, y1, y0, y1}; // q00, q01, q10, q11
            for (int q = 0; q < 4; ++q) {
                const uint32_t *tiled = T.pool.data() + base + tiled_plain(w, 2, 1, nx[q], ny[q]) * 4;
                for (uint32_t k = 0; k < 4; ++k) {
                    CHECK(tiled[k] == ((present & (1u << k)) ? texel(g, k, w, nx[q], ny[q]) : 0u));
                    CHECK(rec[4 * q + k] == tiled[k]);
                }
            }
        }
    // exactly covered: every record of the region is one base texel's, or tile padding that holds zeros
    for (size_t r = 0; r < recs; ++r)
        if (!covered[r]) {
            for (int i = 0; i < 16; ++i)
                CHECK(F.pool[base + r * 16 + i] == 0u);
            for (int i = 0; i < 4; ++i)
                CHECK(T.pool[base + r * 4 + i] == 0u);
        }
    // the cap: a view that would take the scene's footprint records past it is tiled, one that just fits is not
    const Built over = build(g, w, h, present, false, recs * 16 + 99, 100, lead);
    CHECK(over.foot == 100 && over.pool == T.pool);
    for (size_t v = 0; v < over.texs.size(); ++v)
        CHECK(over.texs[v].stride == 4u && over.texs[v].offset == T.texs[v].offset);
    const Built fits = build(g, w, h, present, false, recs * 16 + 100, 100, lead);
    CHECK(fits.foot == 100 + recs * 16 && fits.pool == F.pool && fits.texs[0].stride == RT_TEX_FOOT_STRIDE);
}

int main() {
    const uint32_t sizes[][2] = {{1, 1}, {1, 5}, {2, 2}, {3, 7}, {4, 2}, {5, 3}, {9, 8}, {16, 16}};
    uint32_t g = 0;
    for (const auto &s : sizes) {
        check_size(g, s[0], s[1], 0xFu);
        check_size(g, s[0], s[1], g % 2 ? 0xDu : 0x7u); // an unused slot
        std::printf("size %ux%u ok\n", s[0], s[1]);
        ++g;
    }
    // a scene's sets one after the other against one cap: footprint records while they fit, tiles from the first that does not; a texture on
    // its own is neither (8 x 4 tiles of texels, stride 1) and does not count
    {
        std::vector<uint32_t> pool, a(9 * 8, 0x11111111u);
        std::vector<DevTexture> texs;
        const uint32_t *four[4] = {a.data(), a.data(), nullptr, a.data()}, *one[1] = {a.data()};
        int32_t views[4];
        size_t foot = 0;
        const size_t recs = records_plain(9, 8, 2, 1), cap = 2 * recs * 16 + 15;
        rt::build_texture_views(pool, texs, four, 4u, 9, 8, false, cap, foot, views);
        rt::build_texture_views(pool, texs, one, 1u, 9, 8, false, cap, foot, views);
        CHECK(texs.back().stride == 1u && texs.back().tw_log == 3u && texs.back().th_log == 2u && texs.back().tiles_x == 2u && foot == recs * 16);
        CHECK(pool.size() == texs.back().offset + records_plain(9, 8, 3, 2));
        for (uint32_t y = 0; y < 8; ++y)
            for (uint32_t x = 0; x < 9; ++x)
                CHECK(pool[texs.back().offset + tiled_plain(9, 3, 2, x, y)] == 0x11111111u);
        rt::build_texture_views(pool, texs, four, 4u, 9, 8, false, cap, foot, views);
        CHECK(texs.back().stride == RT_TEX_FOOT_STRIDE && foot == 2 * recs * 16);
        rt::build_texture_views(pool, texs, four, 4u, 9, 8, false, cap, foot, views);
        CHECK(texs.back().stride == 4u && foot == 2 * recs * 16 && texs.size() == 10u);
        for (const DevTexture &t : texs)
            CHECK((t.offset & ~3u) % 32 == 0); // every region starts on a 128-byte boundary; a member's view at its record dword
    }
    std::printf("tex_footprint ok: %llu checks\n", g_checks);
    return 0;
}
