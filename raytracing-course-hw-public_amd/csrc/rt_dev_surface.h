// rt_dev_surface.h — what a hit looks like to shade(): texture sampling and the shading record (to_intersection_info, bvh.h:80-121).
#pragma once
#include "rt_dev_trav.h"

namespace {

// ---------------------------------------------------------------------------------------------- textures
// wrap_repeat geometry.h:517-519: std::fmod(std::fmod(x, 1) + 1, 1) evaluated in DOUBLE (float, int -> double
// overload); fmod(x, 1) == x - trunc(x) exactly.
DEV float wrap_repeat(float x) {
    double xd = (double)x;
    double f = xd - __builtin_trunc(xd);
    double g = f + 1.0;
    double h = g - __builtin_trunc(g);
    return (float)h;
}
DEV int mod_inc(int x, int mod) { return x == mod - 1 ? 0 : x + 1; }

enum { TEX_DEFAULT_WHITE = 0, TEX_DEFAULT_NORMAL_UP = 1 };

DEV DevTexture load_texture(const DevScene &S, int32_t tex) {
    DevTexture T;
    const uint4 *tp = reinterpret_cast<const uint4 *>(S.textures + tex);
    const uint4 t0 = tp[0], t1 = tp[1];
    T.width = t0.x, T.height = t0.y, T.offset = t0.z, T.count = t0.w;
    T.stride = t1.x, T.tiles_x = t1.y, T.tw_log = t1.z, T.th_log = t1.w;
    return T;
}
// tiled index of texel (x, y) within a view
DEV uint32_t tex_tiled(const DevTexture &T, int x, int y) {
    const uint32_t tile = ((uint32_t)y >> T.th_log) * T.tiles_x + ((uint32_t)x >> T.tw_log);
    const uint32_t within = (((uint32_t)y & ((1u << T.th_log) - 1u)) << T.tw_log) | ((uint32_t)x & ((1u << T.tw_log) - 1u));
    return (tile << (T.tw_log + T.th_log)) + within;
}
// The footprint of one bilinear lookup, Texture::sample's address arithmetic (wrap, truncation, neighbours: geometry.h:545-563): the same for
// a texture and for every member of an interleaved view set, which differ only in what at(x, y) loads and which members they blend.
template <class Q> struct Tex4 {
    Q q00, q01, q10, q11;
};
struct TexFoot {
    int w, h;
    int x0, x1, y0, y1;
    float dx, dy;
    DEV TexFoot(const DevTexture &T, float u, float v) {
        float tx = wrap_repeat(u) * (float)T.width;
        float ty = wrap_repeat(v) * (float)T.height;
        int px = (int)tx;
        int py = (int)ty;
        dx = tx - (float)px;
        dy = ty - (float)py;
        w = (int)T.width, h = (int)T.height;
        x0 = px, x1 = mod_inc(px, w), y0 = py, y1 = mod_inc(py, h);
    }
    template <class AT> DEV auto fetch(AT at) const -> Tex4<decltype(at(0, 0))> {
        if (x0 < w && y0 < h)
            return {at(x0, y0), at(x0, y1), at(x1, y0), at(x1, y1)};
        // wrap_repeat rounded up to 1.0f: the reference indexes row-major position x + y*w past the row / the image
        // (geometry.h:556-563); as in the oracle the flat index is clamped for memory safety only, then located
        // Located WITHOUT an integer division (its expansion was the kernel's register-pressure peak, on a path almost no
        // lookup takes): here 0 <= x <= w + 1 and 0 <= y <= h + 1, so the flat index i = x + y * w lies in row y + x / w with
        // x / w in {0, 1, 2}, and an index beyond the last texel is the last texel (w - 1, h - 1).
        auto flat = [&](int x, int y) {
            const int over = x >= 2 * w ? 2 : (x >= w ? 1 : 0);
            int row = y + over, col = x - over * w;
            if (row >= h) { // i > last
                row = h - 1;
                col = w - 1;
            }
            return at(col, row);
        };
        return {flat(x0, y0), flat(x0, y1), flat(x1, y0), flat(x1, y1)};
    }
};
// Decode and bilinear blend of four RGBA8 texels. k/255.0f and powf(k/255.0f, 2.2f) come from the two 256-entry tables staged in LDS
// (bit-identical to the per-lookup arithmetic of geometry.h:525-527, 593-594).
DEV C4 tex_blend(const TexFoot &F, uint32_t a00, uint32_t a01, uint32_t a10, uint32_t a11, bool gamma, const float *s_lin, const float *s_gam) {
    const float *rgb = gamma ? s_gam : s_lin;
    auto dec = [&](uint32_t p) { return C4{rgb[p & 255u], rgb[(p >> 8) & 255u], rgb[(p >> 16) & 255u], s_lin[p >> 24]}; };
    C4 p00 = dec(a00), p01 = dec(a01), p10 = dec(a10), p11 = dec(a11);
    return (1 - F.dx) * ((1 - F.dy) * p00 + F.dy * p01) + F.dx * ((1 - F.dy) * p10 + F.dy * p11);
}

// Texture::sample (geometry.h:545-575). Texels are RGBA8.
template <bool STATS>
DEV C4 tex_sample(const DevScene &S, int32_t tex, int dflt, float u, float v, bool gamma, const float *s_lin, const float *s_gam, LaneStats<STATS> &st) {
    if (tex < 0) {
        if (dflt == TEX_DEFAULT_WHITE)
            return C4{1, 1, 1, 1}; // WHITE_TEXTURE geometry.h:601
        return C4{0.5f, 0.5f, 1, 0}; // NORMAL_UP geometry.h:602
    }
    const DevTexture T = load_texture(S, tex);
    if (T.count == 1) { // 1x1 fast path returns the texel WITHOUT gamma (geometry.h:548-550)
        uint32_t p = S.texels[T.offset];
        return C4{s_lin[p & 255u], s_lin[(p >> 8) & 255u], s_lin[(p >> 16) & 255u], s_lin[p >> 24]};
    }
    const TexFoot F(T, u, v);
    const Tex4<uint32_t> q = F.fetch([&](int x, int y) { return S.texels[T.offset + tex_tiled(T, x, y) * T.stride]; });
    st.texels(4);
    return tex_blend(F, q.q00, q.q01, q.q10, q.q11, gamma, s_lin, s_gam);
}

// The same four lookups when all of a material's textures are members of ONE interleaved view set (DevMaterial::tex_set): equal
// size and tiling, record = {colour, emissive, metallic-roughness, normal} texel at one position. The footprint is the same for every
// member, so it is made once, and each of the four neighbouring records is ONE 16-byte load instead of a 4-byte load per member; every
// member is then decoded and blended with exactly tex_sample's operations in tex_sample's order (tex_blend), so each result is
// bit-identical to the slot-by-slot path.
struct TexSet {
    C4 color, emissive, mr, normal;
};
template <bool STATS>
DEV TexSet tex_sample_set(const DevScene &S, int32_t view, uint32_t info, float u, float v, const float *s_lin, const float *s_gam, LaneStats<STATS> &st) {
    const DevTexture T = load_texture(S, view);
    const uint32_t base = T.offset - ((info >> 4) & 3u); // dword 0 of record (0, 0)
    const TexFoot F(T, u, v);
    // Where the four 16-byte records are (pool dwords); both layouts then run the same four loads, so the branch holds address arithmetic only.
    Tex4<uint32_t> a;
    if (T.stride == RT_TEX_FOOT_STRIDE && F.x0 < F.w && F.y0 < F.h) {
        // a footprint set (rt_tex_views.h): the record of base texel (x0, y0) IS {q00, q01, q10, q11}: one tiled index, four pieces of one line
        const uint32_t rec = base + tex_tiled(T, F.x0, F.y0) * RT_TEX_FOOT_STRIDE;
        a = {rec, rec + 4u, rec + 8u, rec + 12u};
    } else { // an interleaved set; or a footprint set's out-of-range base (TexFoot::fetch), through q00 of the records it names
        a = F.fetch([&](int x, int y) { return base + tex_tiled(T, x, y) * T.stride; });
    }
    auto piece = [&](uint32_t dw) { return *reinterpret_cast<const uint4 *>(S.texels + dw); };
    const Tex4<uint4> q = {piece(a.q00), piece(a.q01), piece(a.q10), piece(a.q11)};
    auto blend = [&](uint32_t a00, uint32_t a01, uint32_t a10, uint32_t a11, bool gamma) {
        st.texels(4);
        return tex_blend(F, a00, a01, a10, a11, gamma, s_lin, s_gam);
    };
    TexSet r;
    r.normal = (info & 8u) ? blend(q.q00.w, q.q01.w, q.q10.w, q.q11.w, false) : C4{0.5f, 0.5f, 1, 0}; // NORMAL_UP geometry.h:602
    r.mr = (info & 4u) ? blend(q.q00.z, q.q01.z, q.q10.z, q.q11.z, false) : C4{1, 1, 1, 1};             // WHITE_TEXTURE geometry.h:601
    r.color = (info & 1u) ? blend(q.q00.x, q.q01.x, q.q10.x, q.q11.x, true) : C4{1, 1, 1, 1};
    r.emissive = (info & 2u) ? blend(q.q00.y, q.q01.y, q.q10.y, q.q11.y, true) : C4{1, 1, 1, 1};
    return r;
}

// ---------------------------------------------------------------------------------------------- shading record
struct Surf { // ray_intersection_info bvh.h:18-29
    V3 normal, shading_normal;
    C4 color;
    V3 emission;
    float metallic, roughness, ior;
};

// to_intersection_info bvh.h:80-121
template <bool STATS>
DEV Surf make_surf(const DevScene &S, const Hit &h, V3 ro, V3 rd, const float *s_lin, const float *s_gam, LaneStats<STATS> &st) {
    if (h.k & RT_PRIM_FLAG) { // analytic primitive: geometric normal only, untextured material (rt_primspec.h)
        const rt_primitive_desc p = load_prim(S.prims, h.k & ~RT_PRIM_FLAG);
        const float oo[3] = {ro.x, ro.y, ro.z}, dd[3] = {rd.x, rd.y, rd.z};
        float t, n[3] = {0.f, 0.f, 1.f};
        (void)rt_prim_intersect(&p, oo, dd, 1e-4f, &t, n); // same inputs as the cast -> same root, same normal
        DevMaterial m;
        {
            const float4 *mp = reinterpret_cast<const float4 *>(S.materials + p.material_id);
            float4 *q = reinterpret_cast<float4 *>(&m);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                q[i] = mp[i];
        }
        st.shaded();
        Surf s;
        s.normal = s.shading_normal = mk(n[0], n[1], n[2]);
        s.color = C4{m.color[0], m.color[1], m.color[2], m.color[3]};
        s.emission = mk(m.emission[0], m.emission[1], m.emission[2]);
        s.metallic = m.metallic;
        s.roughness = m.roughness;
        s.ior = m.ior;
        return s;
    }
    DevAttr at;
    {
        const float4 *p = reinterpret_cast<const float4 *>(S.attrs + h.k);
        float4 *q = reinterpret_cast<float4 *>(&at);
#pragma unroll
        for (int i = 0; i < 7; ++i)
            q[i] = p[i];
    }
    // The material record is read in two halves: the texture slots and scalar factors now, colour / emission / roughness only
    // AFTER the four texture lookups (their registers would otherwise sit idle through the kernel's register-pressure peak).
    // The second read hits the line the first one brought in.
    DevMaterial m;
    const float4 *mat_p = reinterpret_cast<const float4 *>(S.materials + at.material);
    {
        float4 *q = reinterpret_cast<float4 *>(&m);
        q[2] = mat_p[2];
        q[3] = mat_p[3];
    }
    const float b = h.b, c = h.c;
    const float w0 = (1 - b - c); // triangle::interop geometry.h:497-502
    V3 normal = ld3(at.gn);
    bool is_inside = dot(normal, rd) > 0;
    V3 smooth = norm(ld3(at.n) * w0 + ld3(at.n + 3) * b + ld3(at.n + 6) * c);
    if (dot(normal, smooth) < 0)
        smooth = -smooth;
    float tu = at.uv[0] * w0 + at.uv[2] * b + at.uv[4] * c;
    float tv = at.uv[1] * w0 + at.uv[3] * b + at.uv[5] * c;
    V3 tangent = norm(ld3(at.tg) * w0 + ld3(at.tg + 3) * b + ld3(at.tg + 6) * c);
    V3 bitangent = crs(smooth, tangent);
    C4 nt, mr, ct, et;
    V3 shading;
    if (m.tex_set >= 0) { // all lookups of this material in one interleaved set: addresses once, one 16-byte load per neighbour
        const TexSet ts = tex_sample_set(S, m.tex_set, m.tex_set_info, tu, tv, s_lin, s_gam, st);
        nt = ts.normal, mr = ts.mr, ct = ts.color, et = ts.emissive;
        V3 normal_loc = norm(mk(nt.r, nt.g, nt.b) * 2 - 1);
        shading = norm(transform3(normal_loc, tangent, bitangent, smooth));
    } else {
        nt = tex_sample(S, m.normal_tex, TEX_DEFAULT_NORMAL_UP, tu, tv, false, s_lin, s_gam, st); // sample_normal geometry.h:577-582
        V3 normal_loc = norm(mk(nt.r, nt.g, nt.b) * 2 - 1);
        shading = norm(transform3(normal_loc, tangent, bitangent, smooth));
        mr = tex_sample(S, m.mr_tex, TEX_DEFAULT_WHITE, tu, tv, false, s_lin, s_gam, st); // geometry.h:623-626
        ct = tex_sample(S, m.color_tex, TEX_DEFAULT_WHITE, tu, tv, true, s_lin, s_gam, st); // :615-617
        et = tex_sample(S, m.emissive_tex, TEX_DEFAULT_WHITE, tu, tv, true, s_lin, s_gam, st); // :619-621
    }
    st.shaded();
    {
        asm volatile("" : "+v"(mat_p)); // not before this point
        float4 *q = reinterpret_cast<float4 *>(&m);
        q[0] = mat_p[0];
        q[1] = mat_p[1];
    }
    Surf s;
    s.normal = is_inside ? -normal : normal;
    s.shading_normal = is_inside ? -shading : shading;
    s.color = C4{m.color[0], m.color[1], m.color[2], m.color[3]} * ct;
    s.emission = mk(m.emission[0], m.emission[1], m.emission[2]) * mk(et.r, et.g, et.b);
    s.metallic = m.metallic * mr.b;
    s.roughness = m.roughness * mr.g;
    s.ior = m.ior;
    return s;
}

} // namespace
