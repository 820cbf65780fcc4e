"""Scenes and caller rays built to take every branch of the shading path: Texture::sample's footprints, to_intersection_info, shade, vndf_sample,
vndf_pdf, the BRDF, trace_ray and sanitize_nans (csrc/rt_dev_surface.h, csrc/rt_dev_shade.h; DESIGN.md "Shading: which branch a test reaches").

Shared by tests/test_shade_census.py (CPU), tests/test_gpu_shade_branches.py and tests/golden/make_shade_branches_golden.py. Which side of a
branch a ray takes is not assumed: every fixture returns (scene, rays, claimed_slots), and OracleScene.shade_census counts the slots; `require`
turns the counts into the condition the tests assert before they compare anything: every claimed slot is taken by at least MIN_EVENTS samples
of the fixture's own rays.

Every scene lies in and above the plane z = 0 and is looked at from +z (scenegen.look_camera looks down -z). No two triangles are coplanar
and overlapping, so closest hits are unique and every tree kind gives the same bits.

  tex_edges   quads whose texcoords put wrap_repeat on 1.0f (u = -1e-9 rounds up to 1.0f in float), alone in u, alone in v and in both, quads
              across the whole texture and quads on a texel-grid corner; textures 1x4, 4x1, 2x2, 5x3 and 33x17; every case through a material
              whose four slots have four different sizes (tex_sample, slot by slot) and through one whose slots are equal-sized
              (tex_sample_set); one quad of 1x1 textures. Every map is emissive too: with ray_depth = 1 a sample IS emission x texel blend.
  surf_edges  back faces, vertex normals that oppose the geometric one, zero tangents, zero vertex normals, tangents along the normal, and a
              normal map that tilts the shading normal almost into the surface.
  brdf_edges  boxes (faces along +-x, +-y, +-z), a (1,1,1)/sqrt(3) quad and an ellipsoid, one material per object (metallic 0 / 0.5 / 1,
              roughness 0 / 1, ior 1 / 1.5, alpha 0 / 0.5 / 1, black), rays at exact normal incidence and grazing; built without lights, with
              3 lights, with enough lights for wf_shade's global-memory light tables (inner + lights > 96), and with 3 lights under an
              environment map.
  ray_kinds   the 3-light brdf_edges scene with rays of length 0.5 and 3, axis-parallel and plane-parallel directions, origins on a surface
              and inside a closed box, streams and first samples at 0, 2^31 and 2^32 - 1."""
import dataclasses
import os

import numpy as np

ENV_PICTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "envmap", "env.png")
MIN_EVENTS = 16  # a claimed slot is taken by at least this many samples of the fixture's rays
UP = -1e-9       # a texcoord whose wrap_repeat is 0.999999999 in double and 1.0f in float
SEED = 7
SAMPLES = 3           # K of the caller-ray comparisons
CAMERA = (64, 48, 4)  # width, height, samples of the camera renders

TEX_KINDS = ("tex_1x1", "tex_inside", "tex_x1_wraps", "tex_y1_wraps", "tex_u_up_inside", "tex_u_up_last_row", "tex_v_up", "tex_both_up", "tex_w1_x1_is_2")
TEX_SIZES = ((1, 4), (4, 1), (2, 2), (5, 3), (33, 17))  # (width, height)


class _Mesh:
    """Triangles with explicit per-vertex attributes, appended quad by quad."""

    def __init__(self):
        self.pos, self.nrm, self.uv, self.tan, self.mat, self.quads = [], [], [], [], [], []

    def tri(self, p, mat, uv=None, normals=None, tangents=None):
        p = np.asarray(p, dtype=np.float64)
        g = np.cross(p[1] - p[0], p[2] - p[0])
        g /= np.linalg.norm(g)
        self.pos.append(p)
        self.nrm.append(np.tile(g, (3, 1)) if normals is None else np.asarray(normals, dtype=np.float64))
        self.uv.append(np.zeros((3, 2)) if uv is None else np.asarray(uv, dtype=np.float64))
        self.tan.append(np.tile([1.0, 0.0, 0.0], (3, 1)) if tangents is None else np.asarray(tangents, dtype=np.float64))
        self.mat.append(mat)

    def quad(self, p0, e1, e2, mat, uv=((0, 0), (1, 0), (1, 1), (0, 1)), normals=None, tangents=None, reverse=False, name=None):
        """Corners p0, p0 + e1, p0 + e1 + e2, p0 + e2 with texcoords `uv` (and `normals` / `tangents`, 4 x 3) in that order; two triangles that
        share the first corner. `reverse` turns the winding, so the geometric normal is -cross(e1, e2)."""
        p0, e1, e2 = (np.asarray(v, dtype=np.float64) for v in (p0, e1, e2))
        c = np.array([p0, p0 + e1, p0 + e1 + e2, p0 + e2])
        uv = np.asarray(uv, dtype=np.float64)
        for idx in ((0, 1, 2), (0, 2, 3)):
            idx = list(idx if not reverse else (idx[0], idx[2], idx[1]))
            self.tri(c[idx], mat, uv[idx], None if normals is None else np.asarray(normals, dtype=np.float64)[idx],
                     None if tangents is None else np.asarray(tangents, dtype=np.float64)[idx])
        self.quads.append(dict(name=name, p0=p0, e1=e1, e2=e2))

    def scene(self, sg, materials, textures, camera, explicit_normals, **kw):
        f = lambda a: np.asarray(a, dtype=np.float32) + np.float32(0.0)  # noqa: E731
        return sg.Scene(positions=f(self.pos), normals=f(self.nrm) if explicit_normals else None, texcoords=f(self.uv), tangents=f(self.tan),
                        material_ids=np.asarray(self.mat, dtype=np.uint32), materials=materials, textures=textures, camera=camera, **kw)


def _down_rays(quads, per_quad, rng, height=5.0, spread=0.0):
    """`per_quad` rays onto random interior points of each quad, from `height` along the quad's cross(e1, e2) side. spread = 0: orthographic,
    exactly along -cross(e1, e2) (axis-parallel for an axis-parallel quad); otherwise tilted by up to `spread` along e1 and e2."""
    out = []
    for q in quads:
        n = np.cross(q["e1"], q["e2"])
        n /= np.linalg.norm(n)
        s, t = rng.uniform(0.03, 0.97, size=(2, per_quad, 1))
        target = q["p0"] + s * q["e1"] + t * q["e2"]
        d = np.tile(-n, (per_quad, 1))
        if spread:
            a, b = rng.uniform(-spread, spread, size=(2, per_quad, 1))
            d = d + a * q["e1"] / np.linalg.norm(q["e1"]) + b * q["e2"] / np.linalg.norm(q["e2"])
            d /= np.linalg.norm(d, axis=1, keepdims=True)
        out.append(np.concatenate([target - height * d, d], axis=1))
    return np.concatenate(out).astype(np.float32)


def require(what, census, claimed, least=MIN_EVENTS):
    """Assert that every claimed slot was taken at least `least` times; prints the counts (run with -s for the report) and returns them."""
    counts = {k: int(census[k]) for k in claimed}
    print(f"[shade branches] {what}: " + ", ".join(f"{k} {v}" for k, v in counts.items()))
    short = {k: v for k, v in counts.items() if v < least}
    assert not short, f"{what}: claimed slots taken fewer than {least} times: {short}"
    return counts


# ------------------------------------------------------------------------------------------------------------------ tex_edges
def _edge_textures(rng):
    """T[size index][slot]: colour, emissive, metallic-roughness and normal maps of every size in TEX_SIZES, with strong contrast from texel to
    texel (a lookup that reads a neighbour instead shows), colour alpha 255 and normals within about 35 degrees of straight up."""
    textures, index = [], []
    for (w, h) in TEX_SIZES:
        ids = []
        for slot in ("color", "emissive", "mr", "normal"):
            t = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
            if slot == "normal":
                t[..., :2] = rng.integers(70, 186, size=(h, w, 2), dtype=np.uint8)
                t[..., 2] = 255
            if slot == "color":
                t[..., :3] = rng.integers(60, 256, size=(h, w, 3), dtype=np.uint8)
            t[..., 3] = 255
            ids.append(len(textures))
            textures.append(t)
        index.append(ids)
    return textures, index


def tex_edges(sg, depth1=False, reference_safe=False):
    """(scene, rays, claimed). depth1: ray_depth = 1, so a sample is exactly emission x the emissive map's texel blend (or the background);
    otherwise depth 4. reference_safe: without the quads whose lookups pass the last texel of the array ("u up alone" keeps only the rows whose
    whole footprint lies inside, "v up alone" and "both" are dropped): what an implementation that does not clamp the flat index can render."""
    rng = np.random.default_rng(101)
    textures, T = _edge_textures(rng)
    one = len(textures)  # four 1x1 textures: Texture::sample returns the texel before it looks at the coordinates
    for k in range(4):
        textures.append(np.array([[[200 - 40 * k, 90 + 50 * k, 128 if k < 3 else 255, 255]]], dtype=np.uint8))
    textures[one + 3][0, 0] = (140, 120, 255, 255)
    materials = []
    n = len(TEX_SIZES)
    for i in range(n):  # material 2i: four slots of one size (one interleaved set); 2i + 1: four different sizes (slot by slot)
        common = dict(color=(0.9, 0.9, 0.9, 1.0), emission=(1.0, 1.0, 1.0), emissive_strength=1.5, roughness=1.0, metallic=1.0)
        materials.append(sg.Material(color_tex=T[i][0], emissive_tex=T[i][1], metallic_roughness_tex=T[i][2], normal_tex=T[i][3], **common))
        materials.append(sg.Material(color_tex=T[i][0], emissive_tex=T[(i + 1) % n][1], metallic_roughness_tex=T[(i + 2) % n][2], normal_tex=T[(i + 3) % n][3], **common))
    materials.append(sg.Material(color=(0.9, 0.9, 0.9, 1.0), emission=(1.0, 1.0, 1.0), emissive_strength=1.5, roughness=1.0, metallic=1.0,
                                 color_tex=one, emissive_tex=one + 1, metallic_roughness_tex=one + 2, normal_tex=one + 3))
    mesh = _Mesh()
    slot = 0

    def place(mat, uv, name):
        nonlocal slot
        col, row = slot % 8, slot // 8
        slot += 1
        # every quad in a plane of its own (z differs): no two are coplanar
        mesh.quad((1.25 * col, 1.25 * row, 0.01 * (slot % 7)), (1, 0, 0), (0, 1, 0), mat, uv=uv, name=name)

    for i, (w, h) in enumerate(TEX_SIZES):
        for m in (2 * i, 2 * i + 1):
            # reference_safe: the largest index of a "u up alone" footprint is (w + 1) + (py + 1) * w, inside the array for
            # py <= h - 3 (py <= h - 4 for w = 1)
            max_py = h - 3 if w >= 2 else h - 4
            safe_v1 = (max_py + 1) / h
            if not reference_safe:
                place(m, ((UP, 0), (UP, 0), (UP, 0.999), (UP, 0.999)), f"u_up {w}x{h}")
                place(m, ((0, UP), (0.999, UP), (0.999, UP), (0, UP)), f"v_up {w}x{h}")
                place(m, ((UP, UP),) * 4, f"both_up {w}x{h}")
            elif max_py >= 0 and m == 2 * i:  # the equal-sized material only: the other one reads three maps of other heights at the same v
                place(m, ((UP, 0), (UP, 0), (UP, safe_v1 * 0.999), (UP, safe_v1 * 0.999)), f"u_up {w}x{h}")
            place(m, ((0, 0), (0.999, 0), (0.999, 0.999), (0, 0.999)), f"span {w}x{h}")
            place(m, (((w - 1) / w, (h - 1) / h),) * 4, f"corner {w}x{h}")  # on the grid lines of the last texel: px = w - 1, py = h - 1
    place(len(materials) - 1, ((0, 0), (0.999, 0), (0.999, 0.999), (0, 0.999)), "1x1")
    cam = sg.look_camera((4.9, 0.625 * (slot // 8 + 1), 9.5), yaw_deg=0.0, yfov=0.9, aspect=64 / 48)
    sc = mesh.scene(sg, materials, textures, cam, explicit_normals=False, ray_depth=1 if depth1 else 4)
    rays = _down_rays(mesh.quads, 48, np.random.default_rng(102))
    kinds = TEX_KINDS if not reference_safe else ("tex_1x1", "tex_inside", "tex_x1_wraps", "tex_y1_wraps", "tex_u_up_inside")
    claimed = tuple(f"{k}_{g}" for k in kinds for g in ("gamma", "linear")) + ("surf_triangle", "surf_outside", "brdf_metallic_between")
    return sc, rays, claimed


# ------------------------------------------------------------------------------------------------------------------ surf_edges
def surf_edges(sg):
    """(scene, rays, claimed): unit quads in the plane z = 0 (each a little higher than the last), three small lights above them."""
    rng = np.random.default_rng(201)
    tilt = np.zeros((4, 4, 4), dtype=np.uint8)  # a normal map that leans the shading normal ~80 degrees along the tangent
    tilt[..., 0] = rng.integers(244, 256, size=(4, 4))
    tilt[..., 1] = rng.integers(120, 136, size=(4, 4))
    tilt[..., 2] = rng.integers(136, 150, size=(4, 4))
    tilt[..., 3] = 255
    materials = [
        sg.Material(color=(0.8, 0.7, 0.6, 1.0), roughness=0.6, metallic=0.0),
        sg.Material(color=(1.0, 1.0, 1.0, 1.0), emission=(1.0, 0.9, 0.8), emissive_strength=12.0, roughness=1.0, metallic=0.0),
        sg.Material(color=(0.7, 0.8, 0.9, 1.0), roughness=0.8, metallic=0.0, normal_tex=0),
        sg.Material(color=(0.9, 0.9, 0.9, 1.0), roughness=0.0, metallic=1.0),
    ]
    mesh = _Mesh()
    z = np.array([0.0, 0.0, 1.0])
    lean = lambda dx, dy: np.array([dx, dy, 1.0]) / np.linalg.norm([dx, dy, 1.0])  # noqa: E731
    cases = [
        ("front", dict()),
        ("back", dict(reverse=True, normals=[-z] * 4)),                                              # is_inside for a ray from +z
        ("opposed", dict(normals=[-lean(0.2, 0.1), -lean(-0.1, 0.2), -lean(0.1, -0.2), -lean(-0.2, -0.1)])),  # smooth normal flipped
        ("smooth", dict(normals=[lean(0.3, 0.0), lean(0.0, 0.3), lean(-0.3, 0.0), lean(0.0, -0.3)])),  # kept
        ("zero_tangent", dict(tangents=[[0, 0, 0]] * 4)),                                           # norm(0) = NaN tangent
        ("zero_normal", dict(normals=[[0, 0, 0]] * 4)),                                             # NaN smooth normal
        ("tangent_along_normal", dict(tangents=[z] * 4)),                                           # bitangent = 0
        ("tilt_map", dict(mat=2)),
        ("back_opposed", dict(reverse=True, normals=[lean(0.2, 0.1)] * 4)),
        ("tilt_map_back", dict(mat=2, reverse=True, normals=[-z] * 4)),
        # The input for shade's `p < EPS` exit: vertex normals exactly perpendicular to an axis-parallel ray. The shading normal is (1, 0, 0)
        # (the default tangent lies along it, so the bitangent is 0 and the normal map's straight-up texel returns the smooth normal), v.z =
        # -dot(shading normal, in_dir) is exactly 0, lambda = (-1 + sqrt(1 + x / 0)) / 2 is +inf, g1 = 0 and vndf_pdf returns exactly 0. A
        # near-mirror's VNDF direction is in_dir reflected about ~(1, 0, 0), which is in_dir itself: below the geometric horizon, where the
        # cosine density is 0 as well and no light lies. p = 0 < EPS for every sample that takes the VNDF technique.
        ("perpendicular_normal", dict(mat=3, normals=[[1, 0, 0]] * 4)),
    ]
    for k, (name, kw) in enumerate(cases):
        kw = dict(kw)
        mesh.quad((1.5 * (k % 5), 1.5 * (k // 5), 0.02 * k), (1, 0, 0), (0, 1, 0), kw.pop("mat", 0), name=name, **kw)
    quads = list(mesh.quads)
    for c in ((0.5, 3.4, 3.0), (3.5, -0.9, 3.2), (7.4, 1.4, 2.8)):  # lights: small, above and beside the quads, no two in one plane
        c = np.asarray(c)
        mesh.tri([c + [-0.5, -0.3, 0.0], c + [0.5, -0.3, 0.1], c + [0.0, 0.5, 0.2]], 1)
    cam = sg.look_camera((3.5, 1.25, 5.0), yaw_deg=0.0, yfov=0.9, aspect=64 / 48)
    with np.errstate(invalid="ignore", divide="ignore"):
        sc = mesh.scene(sg, materials, [tilt], cam, explicit_normals=True, ray_depth=4)
    rays = np.concatenate([_down_rays(quads[:-1], 160, np.random.default_rng(202), height=2.0, spread=0.35),
                           _down_rays(quads[-1:], 160, np.random.default_rng(203), height=2.0)])  # exactly along -z
    claimed = ("surf_inside", "surf_outside", "surf_smooth_flipped", "surf_smooth_kept", "surf_shading_nan", "surf_shading_finite", "surf_triangle",
               "shade_nan_dir_exit", "shade_dir_finite", "shade_scl_zero_exit", "shade_push", "sanitize_x", "sanitize_y", "sanitize_z",
               "shade_vndf", "shade_mix_cosine", "shade_mix_light", "light_folded", "light_not_folded", "shade_p_lt_eps_exit", "shade_p_ok")
    return sc, rays, claimed


# ------------------------------------------------------------------------------------------------------------------ brdf_edges
BRDF_BUILDS = ("no_lights", "three_lights", "many_lights", "env")
BRDF_MATERIALS = (  # one object each: (name, Material fields)
    ("diffuse", dict(color=(0.8, 0.6, 0.4, 1.0), metallic=0.0, roughness=1.0, ior=1.5)),
    ("mirror", dict(color=(0.9, 0.9, 0.7, 1.0), metallic=1.0, roughness=0.0, ior=1.5)),
    ("half_metal", dict(color=(0.5, 0.8, 0.6, 1.0), metallic=0.5, roughness=0.5, ior=1.5)),
    ("glossy_ior1", dict(color=(0.7, 0.7, 0.9, 1.0), metallic=0.0, roughness=0.0, ior=1.0)),
    ("alpha0", dict(color=(0.9, 0.2, 0.2, 0.0), metallic=0.0, roughness=1.0, ior=1.5)),
    ("alpha_half", dict(color=(0.2, 0.9, 0.2, 0.5), metallic=0.5, roughness=1.0, ior=1.0)),
    ("black", dict(color=(0.0, 0.0, 0.0, 1.0), metallic=0.0, roughness=0.3, ior=1.5)),
    ("rough_metal", dict(color=(0.9, 0.7, 0.3, 1.0), metallic=1.0, roughness=1.0, ior=1.5)),
)
LIGHT_MATERIAL = len(BRDF_MATERIALS)


def _brdf_geometry(sg, build):
    rng = np.random.default_rng(301)
    materials = [sg.Material(**kw) for _, kw in BRDF_MATERIALS]
    materials.append(sg.Material(color=(1.0, 1.0, 1.0, 1.0), emission=(1.0, 0.95, 0.9), emissive_strength=6.0, roughness=1.0, metallic=0.0))
    mesh = _Mesh()
    boxes = []
    for k in range(len(BRDF_MATERIALS)):  # unit boxes on a 3 x 3 grid of pitch 3 (the centre place stays empty), each a little higher than the last
        cell = k if k < 4 else k + 1
        c = np.array([3.0 * (cell % 3), 3.0 * (cell // 3), 0.5 + 0.05 * k])
        for t in sg._box_triangles(c - 0.5, c + 0.5):
            mesh.tri(t, k)
        boxes.append(c)
    # a quad whose normal is (1, 1, 1) / sqrt(3), over the empty centre place
    mesh.quad((2.6, 2.9, 1.2), (0.8, -0.8, 0.0), (0.4, 0.4, -0.8), 2, name="diagonal")
    n_lights = {"no_lights": 0, "three_lights": 3, "many_lights": 100, "env": 3}[build]
    for i in range(n_lights):  # small lights between z = 3.6 and 4.6, random orientation
        c = np.array([rng.uniform(-1.0, 7.0), rng.uniform(-1.0, 7.0), rng.uniform(3.6, 4.6)])
        mesh.tri(c + rng.uniform(-0.45, 0.45, size=(3, 3)), LIGHT_MATERIAL)
    prims = [dict(kind=1, material_id=0, param=(0.6, 0.45, 0.5), position=(3.0, -2.2, 0.7), rotation=(0.0, 0.0, 0.0, 1.0))]
    return mesh, materials, boxes, prims


def _brdf_rays(boxes, rng, normal_per_face=32, grazing_per_face=12):
    rays = []
    for c in boxes:
        for axis in range(3):
            for sign in (-1.0, 1.0):
                n = np.zeros(3)
                n[axis] = sign
                a, b = np.eye(3)[(axis + 1) % 3], np.eye(3)[(axis + 2) % 3]
                k = normal_per_face + grazing_per_face
                s, t = rng.uniform(-0.45, 0.45, size=(2, k, 1))
                target = c + 0.5 * n + s * a + t * b
                d = np.tile(-n, (k, 1))  # exact normal incidence: one component is -+1, the others are 0
                phi = rng.uniform(0, 2 * np.pi, size=(grazing_per_face, 1))
                g = -0.03 * n + np.cos(phi) * a + np.sin(phi) * b  # 1.7 degrees above the face
                d[normal_per_face:] = g / np.linalg.norm(g, axis=1, keepdims=True)
                rays.append(np.concatenate([target - 1.0 * d, d], axis=1))
    return np.concatenate(rays)


def brdf_edges(sg, rt, build):
    """(scene, rays, claimed) of one of BRDF_BUILDS. `rt`: the package (decodes the environment picture for build "env")."""
    assert build in BRDF_BUILDS
    mesh, materials, boxes, prims = _brdf_geometry(sg, build)
    textures, bg_texture = [], -1
    if build == "env":
        textures, bg_texture = [np.ascontiguousarray(rt.image_decode(ENV_PICTURE), dtype=np.uint8)], 0
    cam = sg.look_camera((3.0, 2.4, 11.0), yaw_deg=0.0, yfov=0.9, aspect=64 / 48)
    sc = mesh.scene(sg, materials, textures, cam, explicit_normals=False, ray_depth=3, primitives=prims, bg_texture=bg_texture,
                    bg_color=(0.6, 0.7, 0.8))
    rng = np.random.default_rng(302)
    diag = _down_rays(mesh.quads, 96, rng, height=1.0, spread=0.5)
    # onto the ellipsoid from all round, and from below onto the boxes' undersides with the lights above (many_lights: the huge one)
    e = np.asarray(prims[0]["position"])
    d = rng.normal(size=(96, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ell = np.concatenate([e - 1.5 * d + rng.uniform(-0.2, 0.2, size=(96, 3)), d], axis=1)
    rays = np.concatenate([_brdf_rays(boxes, rng), diag, ell]).astype(np.float32)
    claimed = ("vndf_lensq_zero", "vndf_lensq_pos", "local_x_arm_x", "local_x_arm_y", "local_x_arm_z", "vndf_pdf_vdn_pos",
               "brdf_metallic_0", "brdf_metallic_1", "brdf_metallic_between", "brdf_rough_clamped", "brdf_rough_kept",
               "spec_ndh_one", "spec_hdo_one", "spec_hdi_one",
               "shade_alpha_pass", "shade_alpha_scatter", "shade_vndf", "shade_p_ok", "shade_push", "shade_scl_zero_exit",
               "surf_analytic", "surf_triangle", "surf_inside", "surf_outside", "trace_miss_background", "trace_depth_exhausted")
    if build == "no_lights":
        claimed += ("shade_cosine_no_lights", "tex_1x1_gamma")
    else:
        claimed += ("shade_mix_cosine", "shade_mix_light", "light_folded", "light_not_folded", "spec_ndh_zero")
    if build == "env":
        claimed += ("tex_inside_gamma",)
    return sc, rays, claimed


# ------------------------------------------------------------------------------------------------------------------ ray_kinds
RAY_KIND_OUTPUTS = (1, 4, 7)  # rays_per_output values every ray set divides by
RAY_KIND_SAMPLES = (1, 3)


def ray_kinds(sg, rt, abi):
    """(scene, packed rays, claimed): the three-light brdf_edges scene and rt_ray records (abi.RAY_DTYPE) of every kind the camera never
    makes. Their number is a multiple of 4 x 7. Streams and first samples cycle through 0, 2^31 and 2^32 - 1 (with K = 3 the sample index of
    the last wraps to 0 and 1) and otherwise are random 32-bit numbers."""
    sc, base, _ = brdf_edges(sg, rt, "three_lights")
    rng = np.random.default_rng(401)
    _, _, boxes, _ = _brdf_geometry(sg, "three_lights")
    kinds = []
    short, long_ = base[:560].copy(), base[560:1120].copy()
    short[:, 3:] *= np.float32(0.5)  # unnormalised directions: half and three times unit length
    long_[:, 3:] *= np.float32(3.0)
    kinds += [short, long_]
    # two zero components (axis-parallel) and one zero component (parallel to a coordinate plane), from all over the scene
    o = rng.uniform([-1.5, -3.5, -0.5], [7.5, 7.5, 3.0], size=(560, 3))
    d = np.zeros((560, 3))
    d[np.arange(280), rng.integers(0, 3, 280)] = rng.choice([-1.0, 1.0], 280)
    plane = rng.normal(size=(280, 3))
    plane[np.arange(280), rng.integers(0, 3, 280)] = 0.0
    d[280:] = plane / np.linalg.norm(plane, axis=1, keepdims=True)
    kinds.append(np.concatenate([o, d], axis=1))
    # origins exactly on a face of a box (heading out and heading in) and inside the closed boxes
    on, inside = [], []
    for c in boxes:
        for axis in range(3):
            n = np.zeros(3)
            n[axis] = 1.0
            for _ in range(7):
                p = c + 0.5 * n + rng.uniform(-0.4, 0.4) * np.eye(3)[(axis + 1) % 3] + rng.uniform(-0.4, 0.4) * np.eye(3)[(axis + 2) % 3]
                dd = rng.normal(size=3)
                on.append(np.concatenate([p, dd / np.linalg.norm(dd)]))
        for _ in range(14):
            dd = rng.normal(size=3)
            inside.append(np.concatenate([c + rng.uniform(-0.4, 0.4, size=3), dd / np.linalg.norm(dd)]))
    kinds += [np.asarray(on), np.asarray(inside)]
    od = np.concatenate(kinds).astype(np.float32)
    od = od[: len(od) // 28 * 28]
    packed = np.zeros(len(od), dtype=abi.RAY_DTYPE)
    packed["origin"], packed["dir"] = od[:, :3], od[:, 3:]
    edge = np.array([0, 1 << 31, (1 << 32) - 1], dtype=np.uint64)
    stream = rng.integers(0, 1 << 32, size=len(od), dtype=np.uint64)
    first = rng.integers(0, 1 << 32, size=len(od), dtype=np.uint64)
    stream[::3] = edge[(np.arange(len(od))[::3] // 3) % 3]       # every combination of the edge values occurs
    first[::3] = edge[(np.arange(len(od))[::3] // 9) % 3]
    first[1::3] = edge[(np.arange(len(od))[1::3] // 3) % 3]
    stream[2::3] = edge[(np.arange(len(od))[2::3] // 3) % 3]
    packed["stream"], packed["first_sample"] = stream.astype(np.uint32), first.astype(np.uint32)
    # For unit directions dot(h, out) = dot(h, -in) = dot(-in, h) = (1 - in . out) / |out - in| >= 0: the zero side of those two heaviside
    # factors and vndf_pdf's `vdn <= 0` need an in_dir that is not of unit length, which only a caller's first ray can be.
    claimed = ("surf_inside", "surf_outside", "shade_push", "shade_alpha_pass", "trace_miss_background", "shade_mix_light", "shade_vndf", "vndf_lensq_zero",
               "vndf_pdf_vdn_le_0", "spec_hdo_zero", "spec_hdi_zero")
    return sc, packed, claimed


FIXTURES = ("tex_edges", "tex_edges_depth1", "surf_edges") + tuple(f"brdf_edges_{b}" for b in BRDF_BUILDS)


def make(name, sg, rt):
    """The fixture `name` of FIXTURES: (scene, rays (n, 6) float32, claimed slots)."""
    if name == "tex_edges":
        return tex_edges(sg)
    if name == "tex_edges_depth1":
        return tex_edges(sg, depth1=True)
    if name == "surf_edges":
        return surf_edges(sg)
    assert name.startswith("brdf_edges_"), name
    return brdf_edges(sg, rt, name[len("brdf_edges_"):])


# camera renders of the fixtures claim what their caller rays claim, except what a jittered camera ray cannot do: meet a face exactly along
# its normal (lensq == 0) or exactly at right angles to its vertex normals (surf_edges' input for p < EPS).
CAMERA_UNCLAIMED = ("vndf_lensq_zero", "shade_p_lt_eps_exit")


# ------------------------------------------------------------------------------------------------------------------ reference pins
REFERENCE_RENDER = (32, 24, 4)  # width, height, samples of the stored renders of the unmodified reference (tests/golden/shade_branches/)


def reference_scenes(sg, rt):
    """name -> the part of a fixture scene that a glTF file carries to the unmodified reference (scenegen.write_gltf), in the order of the
    stored renders. What is lost on the way, and therefore stays pinned to the oracle only:
      * tangents (write_gltf emits none; the reference then uses (1, 0, 0)): surf_edges' zero tangents and tangents along the normal;
      * the analytic ellipsoid of brdf_edges, its background colour and environment map (the reference renders a white environment), and every
        ray_depth other than the reference's own 8;
      * on tex_edges, the lookups that pass the last texel of the array, which the reference reads out of bounds: "u up alone" on the last
        rows, "v up alone" and "both" (tex_edges(reference_safe=True) leaves those quads out and keeps "u up alone" on the rows whose whole
        footprint is inside)."""
    return {
        "tex_edges_safe": dataclasses.replace(tex_edges(sg, reference_safe=True)[0], ray_depth=8),
        "surf_edges": dataclasses.replace(surf_edges(sg)[0], ray_depth=8),
        "brdf_edges_three_lights": dataclasses.replace(brdf_edges(sg, rt, "three_lights")[0], ray_depth=8, primitives=[], bg_color=(1.0, 1.0, 1.0)),
        "brdf_edges_many_lights": dataclasses.replace(brdf_edges(sg, rt, "many_lights")[0], ray_depth=8, primitives=[], bg_color=(1.0, 1.0, 1.0)),
    }


_BRDF_REFERENCE_CLAIMS = ("brdf_metallic_0", "brdf_metallic_1", "brdf_metallic_between", "brdf_rough_clamped", "brdf_rough_kept", "shade_alpha_pass",
                          "shade_alpha_scatter", "local_x_arm_x", "local_x_arm_y", "local_x_arm_z", "shade_vndf", "shade_mix_cosine", "shade_mix_light",
                          "light_folded", "light_not_folded", "shade_scl_zero_exit", "shade_push", "surf_inside", "surf_outside")
REFERENCE_CLAIMS = {  # what the stored render of each reference scene takes at least MIN_EVENTS times (the census of that very render)
    "tex_edges_safe": tuple(f"{k}_{g}" for k in ("tex_1x1", "tex_inside", "tex_x1_wraps", "tex_y1_wraps", "tex_u_up_inside", "tex_w1_x1_is_2")
                            for g in ("gamma", "linear")),
    "surf_edges": ("surf_inside", "surf_outside", "surf_smooth_flipped", "surf_smooth_kept", "surf_shading_nan", "surf_shading_finite",
                   "shade_nan_dir_exit", "shade_scl_zero_exit", "shade_push", "sanitize_x", "sanitize_y", "sanitize_z"),
    "brdf_edges_three_lights": _BRDF_REFERENCE_CLAIMS,
    "brdf_edges_many_lights": _BRDF_REFERENCE_CLAIMS,
}


def reference_ppm_name(name):
    w, h, spp = REFERENCE_RENDER
    return f"{name}_{w}x{h}x{spp}.ppm"
