// tests/scene_prepare_host_main.cpp — the host half of rt_create on the CPU, stand-alone (tests/test_scene_prepare_host.py builds it with the
// address and undefined-behaviour sanitizers; it makes no HIP call).
//   (a) rt::assign_texture_views (csrc/rt_tex_views.h) against a restatement of its contract: every view decodes to its texture, tex_set is
//       set exactly when one record group serves every present slot, regions are disjoint and 128-byte aligned, view ids are stable.
//   (b) rt::prepare (csrc/rt_scene_prepare.cpp) on the same cases as whole descriptors over a 12-triangle soup, in the three host build
//       kinds, and the first refusal of descriptors with two planted faults: as text records, compared with tests/golden/prepared_scene.txt.
// `--record` prints the records of (b); `--check FILE` runs (a) and compares (b) with FILE. With -DPREPARE_ONLY part (a) is left out, so
// that the records can be taken from a tree whose rt_tex_views.h has no assign_texture_views yet.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "rt_scene_impl.h"
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

static uint32_t g_rng = 0x2545F491u;
static uint32_t rnd() { return g_rng = g_rng * 1664525u + 1013904223u; }
static float rndf() { return (float)(rnd() >> 8) / 16777216.0f; }

using Slots = std::array<int32_t, 4>;
struct Size {
    uint32_t w, h;
};
static const Size S1{1, 1}, S5{5, 3}, S8{8, 8};
struct Case {
    const char *name;
    std::vector<Size> textures;
    std::vector<Slots> materials;
    int32_t bg = -1;
    bool force_tiled = false;
    bool no_footprints = false; // (a) only: a footprint cap of 0
    bool tiny_budget = false;   // (a) only: an interleave budget of one dword
};
static const std::vector<Case> &cases() {
    static const std::vector<Case> c = {
        {"four_slots_one_size", {S5, S5, S5, S5}, {{0, 1, 2, 3}}},
        {"two_sizes_tie", {S5, S5, S8, S8}, {{0, 2, 1, 3}}},
        {"all_1x1", {S1, S1, S1, S1}, {{0, 1, 2, 3}}},
        {"one_texture", {S8}, {{0, -1, -1, -1}}},
        {"set_starts_at_slot_1", {S8, S8, S8}, {{-1, 0, 1, 2}}},
        {"set_plus_other_size", {S5, S5, S8}, {{0, 1, 2, -1}}},
        {"same_tuple_twice", {S5, S5, S5, S5}, {{0, 1, 2, 3}, {0, 1, 2, 3}}},
        {"shared_texture_two_tuples", {S5, S5, S5, S8}, {{0, 1, 3, -1}, {-1, 3, 0, 2}}},
        {"bg_shared_with_material", {S8}, {{0, -1, -1, -1}}, 0},
        {"bg_alone", {S5}, {}, 0},
        {"force_tiled", {S5, S5, S5, S5}, {{0, 1, 2, 3}}, -1, true},
        {"footprint_cap_0", {S5, S5, S5, S5}, {{0, 1, 2, 3}}, -1, false, true},
        {"budget_below_first_set", {S5, S5, S5, S5}, {{0, 1, -1, -1}, {2, 3, -1, -1}}, -1, false, false, true},
        {"nothing", {}, {}},
    };
    return c;
}
static std::vector<std::vector<uint32_t>> random_texels(const Case &c) {
    std::vector<std::vector<uint32_t>> t(c.textures.size());
    for (size_t i = 0; i < t.size(); ++i) {
        t[i].resize((size_t)c.textures[i].w * c.textures[i].h);
        for (uint32_t &x : t[i])
            x = rnd();
    }
    return t;
}

#ifndef PREPARE_ONLY
// ------------------------------------------------------------------------------------------------ (a)
struct Assigned {
    std::vector<uint32_t> pool;
    std::vector<DevTexture> texs;
    std::vector<DevMaterial> mats; // their four slots name views
    int32_t bg_view = -2;
    Slots view(size_t m) const { return {mats[m].color_tex, mats[m].emissive_tex, mats[m].mr_tex, mats[m].normal_tex}; }
};
static Assigned assign(const Case &c, const std::vector<std::vector<uint32_t>> &texels, size_t n_materials, int32_t bg) {
    std::vector<rt_texture_desc> src(c.textures.size());
    for (size_t i = 0; i < src.size(); ++i)
        src[i] = {c.textures[i].w, c.textures[i].h, reinterpret_cast<const uint8_t *>(texels[i].data())};
    Assigned a;
    a.mats.resize(n_materials);
    for (size_t i = 0; i < n_materials; ++i) {
        DevMaterial &m = a.mats[i] = DevMaterial{};
        m.color_tex = c.materials[i][0], m.emissive_tex = c.materials[i][1], m.mr_tex = c.materials[i][2], m.normal_tex = c.materials[i][3];
        m.tex_set = 12345, m.tex_set_info = 6789u; // (to be overwritten)
    }
    rt::assign_texture_views(src.data(), (uint32_t)src.size(), bg, c.force_tiled, c.no_footprints ? 0 : rt::TEX_FOOT_CAP_DWORDS, c.tiny_budget ? 1 : rt::TEX_SET_BUDGET_DWORDS,
                             a.mats, a.pool, a.texs, a.bg_view);
    return a;
}
// the tiled index and the padded record count written out once more: tiles of 2^tw x 2^th records, row-major tiles, row-major inside a tile
static size_t tiled_plain(uint32_t w, uint32_t tw, uint32_t th, uint32_t x, uint32_t y) {
    const uint32_t TW = 1u << tw, TH = 1u << th;
    return ((size_t)(y / TH) * ((w + TW - 1) / TW) + x / TW) * TW * TH + (size_t)(y % TH) * TW + x % TW;
}
static size_t records_plain(uint32_t w, uint32_t h, uint32_t tw, uint32_t th) {
    const uint32_t TW = 1u << tw, TH = 1u << th;
    return (size_t)((w + TW - 1) / TW) * ((h + TH - 1) / TH) * TW * TH;
}
static void check_view(const Assigned &a, int32_t view, const Size &size, const std::vector<uint32_t> &texels) { // 1: the view decodes to its texture
    CHECK(view >= 0 && (size_t)view < a.texs.size());
    const DevTexture &t = a.texs[view];
    CHECK(t.width == size.w && t.height == size.h && (t.stride == 1u || t.stride == 4u || t.stride == RT_TEX_FOOT_STRIDE));
    CHECK(t.tw_log == (t.stride == 1u ? 3u : 2u) && t.th_log == (t.stride == 1u ? 2u : 1u));
    for (uint32_t y = 0; y < size.h; ++y)
        for (uint32_t x = 0; x < size.w; ++x) {
            CHECK(rt::tex_tiled_index(t, x, y) == tiled_plain(size.w, t.tw_log, t.th_log, x, y));
            const size_t at = t.offset + tiled_plain(size.w, t.tw_log, t.th_log, x, y) * t.stride;
            CHECK(at < a.pool.size() && a.pool[at] == texels[(size_t)y * size.w + x]);
        }
}
static void check_case(const Case &c) {
    const auto texels = random_texels(c);
    const Assigned a = assign(c, texels, c.materials.size(), c.bg);
    CHECK(a.mats.size() == c.materials.size() && a.pool.size() < ((size_t)1 << 32));
    for (size_t i = 0; i < a.mats.size(); ++i) {
        const DevMaterial &m = a.mats[i];
        const Slots view = a.view(i);
        uint32_t present = 0;
        int first = -1;
        bool one_group = true;
        for (int s = 0; s < 4; ++s) {
            const int32_t tex = c.materials[i][s];
            CHECK((tex < 0) == (view[s] < 0));
            if (tex < 0)
                continue;
            check_view(a, view[s], c.textures[tex], texels[tex]);
            present |= 1u << s;
            first = first < 0 ? s : first;
            const DevTexture &t = a.texs[view[s]], &f = a.texs[view[first]];
            one_group = one_group && t.stride >= 4u && t.offset - (uint32_t)s == f.offset - (uint32_t)first;
            CHECK(c.textures[tex].w * c.textures[tex].h != 1 || t.stride == 1u); // a 1x1 texture is never grouped
        }
        // 2: tex_set exactly when every present slot lies in one record group
        CHECK((m.tex_set >= 0) == (present != 0 && one_group));
        if (m.tex_set >= 0)
            CHECK(m.tex_set == view[first] && m.tex_set_info == (present | (uint32_t)first << 4));
        else
            CHECK(m.tex_set == -1 && m.tex_set_info == 0u);
    }
    CHECK((c.bg < 0) == (a.bg_view < 0));
    if (c.bg >= 0) {
        check_view(a, a.bg_view, c.textures[c.bg], texels[c.bg]);
        CHECK(a.texs[a.bg_view].stride == 1u);
    }
    // 3: the regions of the views (a set's members share one) do not overlap, and each starts on a 128-byte boundary
    std::vector<std::pair<size_t, size_t>> regions;
    for (const DevTexture &t : a.texs) {
        const size_t base = t.stride == 1u ? t.offset : t.offset & ~3u;
        regions.push_back({base, base + records_plain(t.width, t.height, t.tw_log, t.th_log) * t.stride});
        CHECK(base % 32 == 0 && regions.back().second <= a.pool.size());
    }
    for (size_t i = 0; i < a.texs.size(); ++i)
        for (size_t j = 0; j < i; ++j) {
            const bool same_region = regions[i] == regions[j] && a.texs[i].stride >= 4u && a.texs[i].stride == a.texs[j].stride;
            CHECK(same_region ? a.texs[i].offset != a.texs[j].offset : (regions[i].second <= regions[j].first || regions[j].second <= regions[i].first));
        }
    // 4: view ids are stable: the same call gives the same answer, and later materials or the bg view change nothing of earlier materials
    const Assigned again = assign(c, texels, c.materials.size(), c.bg);
    CHECK(again.pool == a.pool && again.bg_view == a.bg_view && again.texs.size() == a.texs.size());
    for (size_t n = 0; n <= c.materials.size(); ++n) {
        const Assigned part = assign(c, texels, n, -1);
        CHECK(part.pool.size() <= a.pool.size() && std::equal(part.pool.begin(), part.pool.end(), a.pool.begin()));
        for (size_t i = 0; i < n; ++i)
            CHECK(part.view(i) == a.view(i) && part.mats[i].tex_set == a.mats[i].tex_set && part.mats[i].tex_set_info == a.mats[i].tex_set_info);
    }
    // what the case is about
    const std::string name = c.name;
    auto stride = [&](size_t mat, int slot) { return a.texs[a.view(mat)[slot]].stride; };
    if (name == "four_slots_one_size")
        CHECK(a.mats[0].tex_set == a.view(0)[0] && a.mats[0].tex_set_info == 0xFu && stride(0, 0) == RT_TEX_FOOT_STRIDE && a.texs.size() == 4u);
    if (name == "two_sizes_tie") // the group of the earlier slot wins
        CHECK(stride(0, 0) >= 4u && stride(0, 2) >= 4u && stride(0, 1) == 1u && stride(0, 3) == 1u && a.mats[0].tex_set == -1);
    if (name == "all_1x1" || name == "one_texture")
        CHECK(a.mats[0].tex_set == -1);
    if (name == "set_starts_at_slot_1")
        CHECK(a.mats[0].tex_set == a.view(0)[1] && a.mats[0].tex_set_info == (0xEu | 1u << 4));
    if (name == "set_plus_other_size")
        CHECK(a.mats[0].tex_set == -1 && stride(0, 0) >= 4u && stride(0, 1) >= 4u && stride(0, 2) == 1u);
    if (name == "same_tuple_twice") // the same views, and the pool does not grow
        CHECK(a.view(1) == a.view(0) && a.mats[1].tex_set == a.mats[0].tex_set && a.pool.size() == assign(c, texels, 1, -1).pool.size() && a.texs.size() == 4u);
    if (name == "shared_texture_two_tuples") { // the stand-alone view once, the sets apart
        CHECK(a.view(0)[2] == a.view(1)[1] && stride(0, 2) == 1u && a.texs.size() == 5u);
        CHECK(stride(0, 0) >= 4u && stride(1, 2) >= 4u && a.view(0)[0] != a.view(1)[2]);
    }
    if (name == "bg_shared_with_material")
        CHECK(a.bg_view == a.view(0)[0] && a.texs.size() == 1u);
    if (name == "bg_alone")
        CHECK(a.bg_view == 0 && a.texs.size() == 1u);
    if (name == "force_tiled" || name == "footprint_cap_0")
        CHECK(stride(0, 0) == 4u && a.mats[0].tex_set == a.view(0)[0]);
    if (name == "budget_below_first_set") // later groups stand alone
        CHECK(a.mats[0].tex_set >= 0 && a.mats[1].tex_set == -1 && stride(1, 0) == 1u && stride(1, 1) == 1u);
    if (name == "nothing")
        CHECK(a.pool.empty() && a.texs.empty() && a.bg_view == -1);
    std::printf("views %s ok\n", c.name);
}
#endif

// ------------------------------------------------------------------------------------------------ (b)
static uint64_t fnv(const void *p, size_t bytes, uint64_t h = 0xcbf29ce484222325ull) {
    for (size_t i = 0; i < bytes; ++i)
        h = (h ^ static_cast<const uint8_t *>(p)[i]) * 0x100000001b3ull;
    return h;
}
template <class T> static uint64_t fnv(const std::vector<T> &v, uint64_t h = 0xcbf29ce484222325ull) { return fnv(v.data(), v.size() * sizeof(T), h); }
static uint64_t fnv(const rt::FlatBvh &f) {
    const uint32_t tail[2] = {f.root, f.fast_ok ? 1u : 0u};
    return fnv(tail, sizeof(tail), fnv(f.tris, fnv(f.nodes)));
}

// a case as a whole descriptor: its textures and materials, one more material that emits and has no texture, a soup of 12 triangles
struct Descriptor {
    std::vector<std::vector<uint32_t>> texels;
    std::vector<rt_texture_desc> textures;
    std::vector<rt_material_desc> materials;
    std::vector<float> pos, nrm, uv, tan;
    std::vector<uint32_t> ids;
    std::vector<rt_primitive_desc> prims;
    rt_scene_desc d{};
    Descriptor(const Case &c, uint32_t build_flags) {
        g_rng = 0x9E3779B9u; // every descriptor from the same stream
        texels = random_texels(c);
        for (size_t i = 0; i < texels.size(); ++i)
            textures.push_back({c.textures[i].w, c.textures[i].h, reinterpret_cast<const uint8_t *>(texels[i].data())});
        for (size_t i = 0; i <= c.materials.size(); ++i) {
            rt_material_desc m{};
            for (float &x : m.color)
                x = rndf();
            m.roughness = rndf(), m.metallic = rndf(), m.ior = 1.0f + rndf();
            m.color_tex = m.emissive_tex = m.metallic_roughness_tex = m.normal_tex = -1;
            if (i < c.materials.size())
                m.color_tex = c.materials[i][0], m.emissive_tex = c.materials[i][1], m.metallic_roughness_tex = c.materials[i][2], m.normal_tex = c.materials[i][3];
            else
                m.emission[0] = 3.0f, m.emission[1] = 2.0f, m.emission[2] = 1.0f;
            materials.push_back(m);
        }
        const uint32_t n = 12;
        pos.resize(9 * n), nrm.resize(9 * n), tan.resize(9 * n), uv.resize(6 * n), ids.resize(n);
        for (auto *v : {&pos, &nrm, &tan, &uv})
            for (float &x : *v)
                x = rndf() * 4.0f - 2.0f;
        for (uint32_t i = 0; i < n; ++i)
            ids[i] = i % (uint32_t)materials.size();
        d.abi_version = RT_ABI_VERSION;
        d.n_triangles = n;
        d.ray_depth = 4;
        d.bg_texture = c.bg;
        d.build_flags = build_flags | (c.force_tiled ? (uint32_t)RT_BUILD_TEX_TILED : 0u);
        point();
    }
    void point() { // (after a vector changed)
        d.positions = pos.data(), d.normals = nrm.data(), d.texcoords = uv.data(), d.tangents = tan.data(), d.material_ids = ids.data();
        d.n_materials = (uint32_t)materials.size(), d.materials = materials.data();
        d.n_textures = (uint32_t)textures.size(), d.textures = textures.data();
        d.n_primitives = (uint32_t)prims.size(), d.primitives = prims.data();
    }
};

static void record_case(const Case &c, const char *kind, uint32_t build_flags, std::ostringstream &o) {
    Descriptor D(c, build_flags);
    std::shared_ptr<const rt::PreparedScene> P;
    CHECK(rt::prepare(&D.d, &P) == RT_OK && P && P->geo);
    const rt::PreparedGeometry &G = *P->geo;
    o << "case " << c.name << " " << kind << "\nbg_view " << P->bg_view << "\n";
    for (size_t i = 0; i < P->mats.size(); ++i) {
        const DevMaterial &m = P->mats[i];
        o << "material " << i << " views " << m.color_tex << " " << m.emissive_tex << " " << m.mr_tex << " " << m.normal_tex << " tex_set " << m.tex_set << " info "
          << m.tex_set_info << "\n";
    }
    for (size_t i = 0; i < P->texs.size(); ++i) {
        const DevTexture &t = P->texs[i];
        o << "view " << i << " " << t.width << " " << t.height << " " << t.offset << " " << t.count << " " << t.stride << " " << t.tiles_x << " " << t.tw_log << " "
          << t.th_log << "\n";
    }
    o << std::hex << "pool " << P->pool.size() << " " << fnv(P->pool) << "\nmats " << fnv(P->mats) << " attrs " << fnv(G.attrs) << " flat0 " << fnv(G.flat[0]) << " flat1 "
      << fnv(G.flat[1]) << " laux " << fnv(G.laux) << " wide_nodes " << fnv(G.wide.nodes) << " wide_tris " << fnv(G.wide_tris) << " luts " << fnv(P->lut_gam, fnv(P->lut_lin))
      << std::dec << "\nlights " << G.laux.size() << " wide_depth " << G.wide.depth << "\n";
}

// descriptors with two faults: the first refusal is the one of the earlier check
enum Fault { BAD_MATERIAL_ID, NON_FINITE, BAD_TEXTURE_INDEX, BAD_BG, EMPTY_TEXTURE, BAD_PRIM_LIST, BAD_PRIM_KIND, N_FAULTS };
static const char *const FAULT_NAMES[N_FAULTS] = {"material_id", "non_finite", "texture_index", "bg_texture", "empty_texture", "primitive_list", "primitive_kind"};
static void plant(Descriptor &D, Fault f) {
    if (f == BAD_MATERIAL_ID)
        D.ids[7] = 99;
    else if (f == NON_FINITE)
        D.pos[9 * 5 + 4] = std::numeric_limits<float>::infinity();
    else if (f == BAD_TEXTURE_INDEX)
        D.materials[0].normal_tex = 17;
    else if (f == BAD_BG)
        D.d.bg_texture = 17;
    else if (f == EMPTY_TEXTURE)
        D.textures[1].height = 0;
    else if (f == BAD_PRIM_LIST)
        D.prims.resize(RT_MAX_PRIMITIVES + 1, rt_primitive_desc{RT_PRIM_PLANE, 0, {0, 1, 0}, {0, 0, 0}, {0, 0, 0, 1}});
    else if (f == BAD_PRIM_KIND)
        D.prims.resize(std::max<size_t>(D.prims.size(), 1), rt_primitive_desc{7u, 0, {0, 1, 0}, {0, 0, 0}, {0, 0, 0, 1}});
    D.point();
}
static void record_refusals(std::ostringstream &o) {
    for (int a = 0; a < N_FAULTS; ++a)
        for (int b = a; b < N_FAULTS; ++b) {
            Descriptor D(cases()[0], a % 2 ? RT_BUILD_WIDE : 0u);
            plant(D, (Fault)a);
            plant(D, (Fault)b);
            std::shared_ptr<const rt::PreparedScene> P;
            const int rc = rt::prepare(&D.d, &P);
            CHECK(rc != RT_OK && !P);
            o << "refusal " << FAULT_NAMES[a] << " + " << FAULT_NAMES[b] << ": " << rc << " " << rt::last_error() << "\n";
        }
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if ((mode != "--record" && mode != "--check") || (mode == "--check" && argc < 3)) {
        std::fprintf(stderr, "usage: %s --record | --check FILE\n", argv[0]);
        return 2;
    }
    std::ostringstream o;
    for (const Case &c : cases()) {
        record_case(c, "flat", 0u, o);
        record_case(c, "wide", RT_BUILD_WIDE, o);
        record_case(c, "device", RT_BUILD_DEVICE_LBVH | RT_BUILD_WIDE, o);
    }
    record_refusals(o);
    if (mode == "--record") {
        std::fputs(o.str().c_str(), stdout);
        return 0;
    }
#ifndef PREPARE_ONLY
    for (const Case &c : cases())
        check_case(c);
#endif
    std::ifstream f(argv[2]);
    std::string expected, got, header;
    CHECK(f.good() && std::getline(f, header) && header.rfind("# ", 0) == 0); // the first line says where the records were taken
    std::istringstream mine(o.str());
    size_t lines = 0;
    while (std::getline(f, expected)) {
        CHECK(std::getline(mine, got));
        if (got != expected) {
            std::fprintf(stderr, "record %zu differs:\n  expected: %s\n  got:      %s\n", lines + 1, expected.c_str(), got.c_str());
            return 1;
        }
        ++lines;
    }
    CHECK(!std::getline(mine, got)); // nothing beyond the fixture
    std::printf("prepared_scene ok: %zu records, %llu checks\n", lines, g_checks);
    return 0;
}
