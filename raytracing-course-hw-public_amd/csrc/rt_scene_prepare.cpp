// rt_scene_prepare.cpp — the host half of rt_create: everything it derives from the descriptor WITHOUT a device (no HIP call in this file).
//
// rt::prepare replaces the host work of RaytracerStaticContext(scene) (src/raytracer.h:440-454): both reference-topology BVH builds and their
// flattening (or the wide collapse), shading records, materials, the tiled / interleaved texture pool, tables. Built ONCE per rt_create /
// rt_create_on and uploaded to every GPU of a group (a multi-GPU scene used to repeat all of it per GPU: an 8.5 s single-thread build times
// eight on S-10M). It comes in two halves (rt_scene_impl.h): the geometry half (prepare_geometry), which rt_update_geometry runs again for
// new arrays, and the rest, which a scene keeps for life. rt_scene.cpp puts the result on a device.
#include <cmath>
#include <cstring>
#include <future>

#include "rt_scene_impl.h"
#include "rt_tex_views.h"

namespace {
struct V3h {
    float x, y, z;
};
inline V3h cross_h(V3h a, V3h b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline float len_h(V3h a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
// triangle::normal (geometry.h:477-479) of a record into n[3]; returns the length of the cross product (twice the area)
inline float unit_normal(const DevTri &tr, float *n) {
    const V3h c = cross_h({tr.v[0], tr.v[1], tr.v[2]}, {tr.u[0], tr.u[1], tr.u[2]});
    const float l = len_h(c);
    n[0] = c.x / l, n[1] = c.y / l, n[2] = c.z / l;
    return l;
}
} // namespace

// ---------------------------------------------------------------------------------------------- the geometry half
// shading records in the order of the triangle records `tris` (to_intersection_info's inputs, bvh.h:80-121)
void rt::make_attrs(const rt_scene_desc *d, const std::vector<DevTri> &tris, std::vector<DevAttr> &attrs) {
    attrs.resize(tris.size());
    for (size_t k = 0; k < attrs.size(); ++k) {
        const uint32_t t = tris[k].prim;
        DevAttr &a = attrs[k];
        std::memset(&a, 0, sizeof(a));
        std::memcpy(a.n, d->normals + 9 * (size_t)t, 36);
        std::memcpy(a.tg, d->tangents + 9 * (size_t)t, 36);
        std::memcpy(a.uv, d->texcoords + 6 * (size_t)t, 24);
        unit_normal(tris[k], a.gn);
        a.material = d->material_ids[t];
    }
}
// triangle records of the wide tree: the reference's operands a, b - a, c - a (geometry.h:473-475) in the tree's own order
void rt::make_wide_tris(const rt_scene_desc *d, const rt::WideBvh &wide, std::vector<DevTri> &tris) {
    tris.resize(wide.order.size());
    for (size_t k = 0; k < tris.size(); ++k) {
        const float *p = d->positions + 9 * (size_t)wide.order[k];
        DevTri &t = tris[k];
        for (int c = 0; c < 3; ++c) {
            t.a[c] = p[c];
            t.v[c] = p[3 + c] - p[c];
            t.u[c] = p[6 + c] - p[c];
        }
        t.prim = wide.order[k];
        t.flags = 0;
        t.pad = 0;
    }
}

// Everything that follows from the five per-triangle arrays of `d` (and from which materials emit). `d` needs n_triangles, the five arrays,
// build_flags and nothing else: rt_update_geometry passes a descriptor of just those.
void rt::prepare_geometry(const rt_scene_desc *d, const std::vector<uint8_t> &emissive, float wide_cost_node, float wide_cost_tri, rt::PreparedGeometry &P,
                          bool lights_only) {
    const uint32_t n = d->n_triangles;
    // ---- RaytracerStaticContext: scene_bvh over everything, light_bvh over emission != 0 (raytracer.h:441-447)
    std::vector<uint32_t> all(n), lights;
    for (uint32_t i = 0; i < n; ++i) {
        all[i] = i;
        if (emissive[d->material_ids[i]])
            lights.push_back(i);
    }
    const rt::BuildKind kind = rt::build_kind(d->build_flags, n);
    const auto tb0 = std::chrono::steady_clock::now();
    if (!kind.dev_build && !lights_only) {
        P.host_bvh[0] = rt::build_bvh(d->positions, n, all);
        if (!kind.wide_build) {
            P.flat[0] = rt::flatten_bvh(P.host_bvh[0], d->positions);
            make_attrs(d, P.flat[0].tris, P.attrs);
        }
        P.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count();
        if (kind.wide_build) { // production build: collapse the reference-topology tree into the 8-wide quantised tree
            const auto tw0 = std::chrono::steady_clock::now();
            P.wide = rt::build_wide(rt::bin_from_host(P.host_bvh[0]), d->positions, wide_cost_node, wide_cost_tri);
            make_wide_tris(d, P.wide, P.wide_tris);
            make_attrs(d, P.wide_tris, P.attrs);
            P.wide_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
        }
    }
    rt::prepare_lights(d->positions, n, lights, nullptr, P);
}

// The light half of prepare_geometry: the reference-topology tree over the triangles `lights` of `positions` (ascending indices into it),
// flattened, and the light records. `original` (rt_update_geometry_device): `positions` holds only the emissive triangles, compacted in
// ascending order of their scene indices original[k], and `lights` is 0, 1, 2, ...: the builder sees the same boxes and centres in the same
// order, so the tree is the one it builds over the whole array, and only the names it stores (HostBvh::order, DevTri::prim) need mapping back.
void rt::prepare_lights(const float *positions, uint32_t n_total, const std::vector<uint32_t> &lights, const uint32_t *original, rt::PreparedGeometry &P) {
    P.host_bvh[1] = rt::build_bvh(positions, n_total, lights);
    P.flat[1] = rt::flatten_bvh(P.host_bvh[1], positions);
    if (original) {
        for (uint32_t &t : P.host_bvh[1].order)
            t = original[t];
        for (DevTri &tr : P.flat[1].tris)
            tr.prim = original[tr.prim];
    }
    P.laux.resize(P.flat[1].tris.size());
    for (size_t k = 0; k < P.laux.size(); ++k)
        P.laux[k].area = unit_normal(P.flat[1].tris[k], P.laux[k].normal) / 2; // triangle::square geometry.h:481-483
}

// ---------------------------------------------------------------------------------------------- the steps of rt::prepare, in its order
// Material ids in range, then vertex positions finite. The reference sorts centroids with std::sort (bvh.h:283-291), which is undefined for
// NaN, and an infinite box poisons every surface-area cost with inf - inf; the device builders (Morton codes, nearest-neighbour search) have
// no meaningful answer either. Refused before any builder or kernel sees them (normals / texcoords / tangents may hold anything).
int rt::check_geometry_contents(const uint32_t *material_ids, const float *positions, uint32_t n, size_t n_materials, const std::string &fn) {
    for (uint32_t i = 0; i < n; ++i)
        if (material_ids[i] >= n_materials)
            return rt::refuse_material(fn);
    for (size_t i = 0; i < (size_t)n * 9; ++i)
        if (!std::isfinite(positions[i]))
            return rt::refuse_non_finite(fn, i / 9);
    return RT_OK;
}

// what the descriptor's arrays may not hold: geometry first, then the texture indices and the textures
static int check_contents(const rt_scene_desc *d) {
    if (int rc = rt::check_geometry_contents(d->material_ids, d->positions, d->n_triangles, d->n_materials, "rt_create"); rc != RT_OK)
        return rc;
    auto tex_ok = [&](int32_t t) { return t < 0 || (uint32_t)t < d->n_textures; };
    for (uint32_t i = 0; i < d->n_materials; ++i) {
        const rt_material_desc &m = d->materials[i];
        if (!tex_ok(m.color_tex) || !tex_ok(m.emissive_tex) || !tex_ok(m.metallic_roughness_tex) || !tex_ok(m.normal_tex))
            return rt::fail(RT_ERR_INVALID_ARG, "rt_create: texture index out of range");
    }
    if (!tex_ok(d->bg_texture))
        return rt::fail(RT_ERR_INVALID_ARG, "rt_create: bg_texture out of range");
    for (uint32_t i = 0; i < d->n_textures; ++i)
        if (d->textures[i].width == 0 || d->textures[i].height == 0 || !d->textures[i].rgba8)
            return rt::fail(RT_ERR_INVALID_ARG, "rt_create: empty texture");
    return RT_OK;
}

std::vector<uint8_t> rt::emissive_materials(const std::vector<DevMaterial> &mats) {
    std::vector<uint8_t> em(mats.size());
    for (size_t i = 0; i < em.size(); ++i) {
        const float *e = mats[i].emission;
        em[i] = !((e[0] == 0) & (e[1] == 0) & (e[2] == 0));
    }
    return em;
}

// the material records; their four texture slots still name textures of the descriptor
static void make_materials(const rt_scene_desc *d, std::vector<DevMaterial> &mats) {
    mats.resize(d->n_materials);
    for (uint32_t i = 0; i < d->n_materials; ++i) {
        const rt_material_desc &m = d->materials[i];
        DevMaterial &o = mats[i];
        std::memset(&o, 0, sizeof(o));
        std::memcpy(o.color, m.color, 16);
        std::memcpy(o.emission, m.emission, 12);
        o.roughness = m.roughness;
        o.metallic = m.metallic;
        o.ior = m.ior;
        o.color_tex = m.color_tex;
        o.emissive_tex = m.emissive_tex;
        o.mr_tex = m.metallic_roughness_tex;
        o.normal_tex = m.normal_tex;
    }
}

// the texel pool and its views (rt_tex_views.h decides both); the materials' slots are remapped to views
static int assign_views(const rt_scene_desc *d, rt::PreparedScene &P) {
    rt::assign_texture_views(d->textures, d->n_textures, d->bg_texture, (d->build_flags & RT_BUILD_TEX_TILED) != 0, rt::TEX_FOOT_CAP_DWORDS, rt::TEX_SET_BUDGET_DWORDS,
                             P.mats, P.pool, P.texs, P.bg_view);
    if (P.pool.size() >= ((size_t)1 << 32))
        return rt::fail(RT_ERR_OOM, "rt_create: texture pool exceeds 2^32 texels");
    return RT_OK;
}

// analytic primitives of the scene-txt front end (rt_primspec.h)
static int copy_primitives(const rt_scene_desc *d, std::vector<rt_primitive_desc> &prims) {
    if (!d->n_primitives)
        return RT_OK;
    if (!d->primitives || d->n_primitives > RT_MAX_PRIMITIVES)
        return rt::fail(RT_ERR_INVALID_ARG, "rt_create: bad primitive list (limit " + std::to_string(RT_MAX_PRIMITIVES) + ")");
    prims.assign(d->primitives, d->primitives + d->n_primitives);
    for (const rt_primitive_desc &pr : prims)
        if ((pr.kind != RT_PRIM_ELLIPSOID && pr.kind != RT_PRIM_PLANE) || pr.material_id >= d->n_materials)
            return rt::fail(RT_ERR_INVALID_ARG, "rt_create: primitive with unknown kind or material id out of range");
    return RT_OK;
}

static void fill_luts(std::vector<float> &lut_lin, std::vector<float> &lut_gam) {
    lut_lin.resize(256);
    lut_gam.resize(256);
    for (int k = 0; k < 256; ++k) {
        lut_lin[k] = k / 255.0f;                 // Texture::load_img geometry.h:593-594
        lut_gam[k] = std::pow(lut_lin[k], 2.2f); // rgba_apply_gamma geometry.h:525-527 (float powf)
    }
}

int rt::prepare(const rt_scene_desc *d, std::shared_ptr<const rt::PreparedScene> *out) {
    auto prepared = std::make_shared<rt::PreparedScene>();
    rt::PreparedScene &P = *prepared;
    if (int rc = check_contents(d); rc != RT_OK)
        return rc;
    P.wide_cost_node = d->build.wide_cost_node > 0.0f ? d->build.wide_cost_node : P.wide_cost_node; // 0 = the default
    P.wide_cost_tri = d->build.wide_cost_tri > 0.0f ? d->build.wide_cost_tri : P.wide_cost_tri;
    P.build_flags = d->build_flags;
    P.build = d->build;
    make_materials(d, P.mats);
    const std::vector<uint8_t> emissive = rt::emissive_materials(P.mats);
    // The geometry half — both BVH builds, flattening or the wide collapse, shading records — runs on a thread of its own while
    // this thread lays out the texture pool below (SURVEY 8f-2 "overlap"): on S-sponza the two halves take about as long as
    // each other (BVH 0.10 s; the texel pool 0.2 s for 268 MB of interleaved sets, more for the 1.07 GB of footprint sets: profiles/shade_lines.txt).
    auto G = std::make_shared<rt::PreparedGeometry>();
    auto geometry_task = std::async(std::launch::async, [&]() { rt::prepare_geometry(d, emissive, P.wide_cost_node, P.wide_cost_tri, *G); });
    struct JoinGeometry { // every return below must wait for the task: it works on `G` and on locals of this frame
        std::future<void> &f;
        ~JoinGeometry() {
            if (f.valid())
                f.wait();
        }
    } join_geometry{geometry_task};

    if (int rc = assign_views(d, P); rc != RT_OK)
        return rc;
    if (int rc = copy_primitives(d, P.prims); rc != RT_OK)
        return rc;
    fill_luts(P.lut_lin, P.lut_gam);
    geometry_task.get();
    P.geo = G;
    *out = prepared;
    return RT_OK;
}
