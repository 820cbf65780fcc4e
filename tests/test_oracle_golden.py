"""Pins the CPU oracle (oracle/rt_oracle.cpp) and the host loader against golden vectors manufactured from the
UNMODIFIED reference (tests/golden/make_golden.py). CPU only.

Parity chain, hop 1: oracle in reference-RNG mode + libm sin/cos == the reference binary, byte for
byte in the PPM, bit for bit in BVH nodes, closest hits (prim, b, c, t) and light pdf values.
"""
import hashlib
import os

import numpy as np
import pytest

import deep_walks
from conftest import golden_scene_specs, make_scene

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIVE = os.path.join(GOLD, "live")  # the reference's answers for the "live" tests below (make_live_golden.py)
GENERATED = list(golden_scene_specs().keys())
# "features": hand-built glTF committed under tests/golden/features/ (scene selection, matrix + TRS nodes, strips,
# u8/u16/u32 indices, missing attributes, lower-case `tangent`, emissive texture + strength, ...; make_features_gltf.py)
NAMES = GENERATED + ["features"]
W, H, SPP = 64, 48, 4


@pytest.fixture(scope="module")
def loaded(rt, sg, tmp_path_factory):
    """Each golden scene written as glTF and read back through the C++ host loader (no GPU involved)."""
    out = {}
    d = tmp_path_factory.mktemp("gltf")
    for name, spec in golden_scene_specs().items():
        sc = make_scene(sg, spec)
        path = sg.write_gltf(sc, str(d / (name + ".gltf")))
        out[name] = (rt.parse_gltf_scene(path, W / H), sc, path)
    path = os.path.join(GOLD, "features", "features.gltf")
    out["features"] = (rt.parse_gltf_scene(path, W / H), None, path)
    return out


@pytest.fixture(scope="module")
def oracles(oracle, loaded):
    return {name: oracle.OracleScene(ls) for name, (ls, _, _) in loaded.items()}


def gold(name):
    return np.load(os.path.join(GOLD, f"{name}_probe.npz"))


@pytest.mark.parametrize("name", NAMES)
def test_loader_matches_reference_scene_objects(loaded, name):
    """C++ glTF loader == parse_gltf_scene (scene.h:183): every triangle attribute and the camera, bit for bit."""
    ls, _, _ = loaded[name]
    a = ls.arrays()
    g = gold(name)
    n = a["positions"].shape[0]
    assert n == g["obj_positions"].shape[0]
    assert np.array_equal(a["positions"].reshape(n, 9).view(np.uint32), g["obj_positions"].view(np.uint32))
    assert np.array_equal(a["normals"].reshape(n, 9).view(np.uint32), g["obj_normals"].view(np.uint32))
    assert np.array_equal(a["texcoords"].reshape(n, 6).view(np.uint32), g["obj_texcoords"].view(np.uint32))
    assert np.array_equal(a["tangents"].reshape(n, 9).view(np.uint32), g["obj_tangents"].view(np.uint32))
    cam = np.concatenate([a["camera"]["position"], a["camera"]["right"], a["camera"]["up"], a["camera"]["forward"], [a["camera"]["fov_x"]]]).astype(np.float32)
    assert np.array_equal(cam.view(np.uint32), g["camera"].view(np.uint32))


@pytest.mark.parametrize("name", GENERATED)
def test_loader_matches_python_generator(loaded, rt, name):
    """The direct-ABI path (numpy arrays -> rt_scene_desc, used by bench.py) feeds the same triangles as the glTF path."""
    ls, sc, _ = loaded[name]
    a = ls.arrays()
    n = sc.n_triangles
    assert np.array_equal(a["positions"].view(np.uint32), sc.positions.astype(np.float32).view(np.uint32))
    assert np.array_equal(a["normals"].view(np.uint32), sc.resolved_normals().view(np.uint32))
    assert np.array_equal(a["texcoords"].view(np.uint32), sc.texcoords.astype(np.float32).view(np.uint32))
    used = sorted(set(int(m) for m in sc.material_ids))
    # glTF materials are converted lazily in order of first use; compare through the per-triangle indirection
    for t in range(0, n, max(1, n // 50)):
        gm = a["materials"][int(a["material_ids"][t])]
        pm = sc.materials[int(sc.material_ids[t])]
        assert np.array_equal(gm["color"], np.asarray(pm.color, dtype=np.float32))
        assert np.array_equal(gm["emission"], pm.emission_f32())
        assert gm["roughness"] == np.float32(pm.roughness) and gm["metallic"] == np.float32(pm.metallic)
        assert (gm["color_tex"], gm["normal_tex"], gm["metallic_roughness_tex"], gm["emissive_tex"]) == (pm.color_tex, pm.normal_tex, pm.metallic_roughness_tex, pm.emissive_tex)
    assert len(used) >= 2
    for i, t in enumerate(sc.textures):
        assert np.array_equal(a["textures"][i], t)
    for k in ("position", "right", "up", "forward"):
        assert np.array_equal(a["camera"][k], np.asarray(getattr(sc.camera, k), dtype=np.float32)), k


@pytest.mark.parametrize("name", NAMES)
def test_oracle_bvh_matches_reference(oracles, name):
    """BVH::build (bvh.h:368-393): node boxes, links, leaf ranges and the object permutation, for both BVHs."""
    g = gold(name)
    for which, tag in ((0, "scene"), (1, "light")):
        b = oracles[name].bvh_info(which)
        assert b["root"] == int(g[f"{tag}_root"])
        assert np.array_equal(b["order"], g[f"{tag}_order"])
        assert np.array_equal(b["nodes"], g[f"{tag}_nodes"])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_closest_hits_match_reference(oracles, name):
    """BVH::intersect_ray (bvh.h:195-235): bit-exact (prim, b, c, t) for pixel-centre rays and random rays."""
    g = gold(name)
    for rays, prim, bct in ((g["primary_rays"], g["primary_prim"], g["primary_bct"]), (g["cast_rays"], g["cast_prim"], g["cast_bct"])):
        p, b = oracles[name].cast_rays(rays)
        assert np.array_equal(p, prim)
        assert np.array_equal(b.view(np.uint32), bct.view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_light_pdf_matches_reference(oracles, name):
    """bvh_mix_dist::pdf (raytracer.h:363-375) through foreach_intersection (bvh.h:237-260)."""
    g = gold(name)
    got = oracles[name].light_pdf(g["cast_rays"])
    assert np.array_equal(got.view(np.uint32), g["light_pdf"].view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_ppm_byte_identical_to_reference(oracles, oracle, rt, name, tmp_path):
    """run_raytracer + Image::set_pixel + Image::write: the PPM the reference binary produced, byte for byte."""
    fb, st = oracles[name].run_raytracer(W, H, SPP, rng_mode=rt.RT_RNG_REFERENCE)
    img = oracle.tonemap(fb)
    ref = oracle.read_ppm(os.path.join(GOLD, f"{name}_{W}x{H}x{SPP}.ppm"))
    assert img.shape == ref.shape
    assert np.array_equal(img, ref), f"{int((img != ref).any(axis=2).sum())} pixels differ"
    # the product's host film + PPM writer produce the same file
    out = tmp_path / "o.ppm"
    rt.write_ppm(str(out), rt.tonemap(fb))
    assert out.read_bytes() == open(os.path.join(GOLD, f"{name}_{W}x{H}x{SPP}.ppm"), "rb").read()
    assert st["samples"] == W * H * SPP


@pytest.mark.parametrize("name", NAMES)
def test_product_host_bvh_builder_matches_reference(rt, loaded, name):
    """The product's own builder (csrc/bvh_build.cpp, what rt_create uploads) against the reference's BVH dump."""
    ls, sc, _ = loaded[name]
    g = gold(name)
    a = ls.arrays()
    b = rt.bvh_build_host(a["positions"])
    assert b["root"] == int(g["scene_root"])
    assert np.array_equal(b["nodes"], g["scene_nodes"]) and np.array_equal(b["order"], g["scene_order"])
    lights = np.array([i for i, m in enumerate(a["material_ids"]) if np.any(a["materials"][int(m)]["emission"] != 0)], dtype=np.uint32)
    bl = rt.bvh_build_host(a["positions"], lights)
    assert np.array_equal(bl["nodes"], g["light_nodes"]) and np.array_equal(bl["order"], g["light_order"])


def test_parallel_subtree_build_is_bit_identical(rt, sg, oracle, monkeypatch):
    """Above 65 536 triangles the product's builder AND the oracle split the top of the tree into parallel tasks; node
    numbering, boxes and the object permutation must equal the sequential, literal oracle build (plain build_node)."""
    sc = sg.room_scene(150000, seed=3, n_lights=8, tex_size=0)
    b = rt.bvh_build_host(sc.positions)
    monkeypatch.setenv("RTO_BUILD_PARALLEL_LEVELS", "0")
    ob = oracle.OracleScene(sc).bvh_info(0)
    monkeypatch.setenv("RTO_BUILD_PARALLEL_LEVELS", "4")
    op = oracle.OracleScene(sc).bvh_info(0)
    assert b["root"] == ob["root"] == op["root"]
    assert np.array_equal(b["nodes"], ob["nodes"]) and np.array_equal(b["order"], ob["order"])
    assert np.array_equal(op["nodes"], ob["nodes"]) and np.array_equal(op["order"], ob["order"])
    leaves = b["nodes"][b["nodes"][:, 6] == 0xFFFFFFFF]
    assert (leaves[:, 9] - leaves[:, 8]).sum() == sc.n_triangles


def reference_ppm(oracle, gltf, w, h, spp, tmp_path, name):
    """The reference binary's PPM of a scene, stored as tests/golden/live/<name> (make_live_golden.py); where oracle/_ref exists the
    binary runs live as well and must reproduce the stored bytes."""
    stored = oracle.read_ppm(os.path.join(LIVE, name))
    if oracle.have_reference_build():
        assert np.array_equal(oracle.run_reference(gltf, w, h, spp, str(tmp_path / "ref.ppm")), stored), name
    return stored


def test_live_reference_bvh_dump_at_100k_if_present(oracle, rt, sg, tmp_path):
    """The reference's own BVH::build (through oracle/_ref/ref_probe) on 100 000 triangles against the oracle's parallel
    build and the product's host builder: nodes and object order bit for bit. The reference's dump is stored as its sha256
    (tests/golden/live/bvh_room100k.sha256); where oracle/_ref exists the dump is also made live and checked against it."""
    sc = sg.room_scene(100000, seed=99, n_lights=20, n_materials=4, tex_size=0, offset=0.05)
    path = sg.write_gltf(sc, str(tmp_path / "big.gltf"))
    stored = open(os.path.join(LIVE, "bvh_room100k.sha256")).read().split()[0]
    if oracle.have_reference_build():
        oracle.ref_probe("bvh", path, 64, 48, str(tmp_path / "bvh.bin"))
        assert hashlib.sha256(np.fromfile(str(tmp_path / "bvh.bin"), dtype=np.uint32).tobytes()).hexdigest() == stored
    ls = rt.parse_gltf_scene(path, 64 / 48)
    orc = oracle.OracleScene(ls)
    a = ls.arrays()
    lights = np.array([i for i, m in enumerate(a["material_ids"]) if np.any(a["materials"][int(m)]["emission"] != 0)], dtype=np.uint32)
    words = []  # the oracle's trees in the layout of the reference's dump: node count, object count, root, nodes, object order
    for which, sub in ((0, None), (1, lights)):
        ob = orc.bvh_info(which)
        pb = rt.bvh_build_host(a["positions"], sub)
        nn, no = len(ob["nodes"]), len(ob["order"])
        assert ob["root"] == pb["root"]
        assert np.array_equal(pb["nodes"], ob["nodes"]) and np.array_equal(pb["order"], ob["order"]), which
        words += [np.array([nn, no, ob["root"]], dtype=np.uint32), np.asarray(ob["nodes"], dtype=np.uint32).reshape(-1), np.asarray(ob["order"], dtype=np.uint32)]
    assert hashlib.sha256(np.concatenate(words).tobytes()).hexdigest() == stored
    assert nn > 1  # 20 lights: a light BVH with inner nodes


def test_oracle_thread_count_does_not_change_the_image(oracles, rt):
    a, _ = oracles["room_plain"].run_raytracer(W, H, 2, rng_mode=rt.RT_RNG_REFERENCE, threads=1)
    b, _ = oracles["room_plain"].run_raytracer(W, H, 2, rng_mode=rt.RT_RNG_REFERENCE, threads=7)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_oracle_sharding_union(oracles, rt):
    full, _ = oracles["boxes"].run_raytracer(W, H, 2, seed=5)
    fb = np.full((H, W, 3), -1, dtype=np.float32)
    for r in range(3):
        oracles["boxes"].run_raytracer(W, H, 2, seed=5, shard_index=r, shard_count=3, shard_block=256, out=fb)
    assert np.array_equal(fb.view(np.uint32), full.view(np.uint32))


def test_live_reference_binary_if_present(oracle, rt, sg, tmp_path):
    """The reference binary on a scene outside the golden_scene_specs set, at another image shape: its PPM is stored
    (tests/golden/live/), and where oracle/_ref exists the binary runs live too."""
    sc = sg.room_scene(900, seed=777, n_lights=5, n_materials=7, tex_size=8, n_tex_sets=3, alpha_fraction=0.3, smooth_normals=True)
    path = sg.write_gltf(sc, str(tmp_path / "live.gltf"))
    ref = reference_ppm(oracle, path, 40, 56, 3, tmp_path, "room900_40x56x3.ppm")
    ls = rt.parse_gltf_scene(path, 40 / 56)
    orc = oracle.OracleScene(ls)
    fb, _ = orc.run_raytracer(40, 56, 3, rng_mode=rt.RT_RNG_REFERENCE)
    assert np.array_equal(oracle.tonemap(fb), ref)


def test_live_reference_binary_on_a_deep_tree_if_present(oracle, rt, sg, tmp_path):
    """Same as above at 30 000 triangles (a BVH ~20 levels deep, textured, dense overlaps): the oracle's PPM must still be
    byte-identical to the reference binary's (stored under tests/golden/live/; live as well where oracle/_ref exists)."""
    sc = sg.room_scene(30000, seed=4711, n_lights=6, n_materials=12, tex_size=16, n_tex_sets=4, alpha_fraction=0.1, offset=0.4)
    path = sg.write_gltf(sc, str(tmp_path / "deep.gltf"))
    ref = reference_ppm(oracle, path, 96, 64, 2, tmp_path, "room30000_96x64x2.ppm")
    ls = rt.parse_gltf_scene(path, 96 / 64)
    fb, _ = oracle.OracleScene(ls).run_raytracer(96, 64, 2, rng_mode=rt.RT_RNG_REFERENCE)
    assert np.array_equal(oracle.tonemap(fb), ref)


# Hop 1 of the parity chain on the trees of tests/test_gpu_deep_walks.py: everything above stops at 40 coplanar lights and at light queries
# with 3 subtrees pending. The scenes are tests/deep_walks.py's; the reference's answers are stored by make_live_golden.py.
def test_live_reference_binary_with_2000_volume_lights_if_present(oracle, rt, sg, tmp_path):
    """2000 emissive triangles all through the room (a light tree of 2555 pieces; most light queries keep 5 to 11 subtrees pending): the
    oracle's PPM is the reference binary's, byte for byte."""
    sc = deep_walks.volume_lights_scene(sg, **deep_walks.BIG_LIGHTS)
    path = sg.write_gltf(sc, str(tmp_path / "lights.gltf"))
    ref = reference_ppm(oracle, path, 48, 40, 2, tmp_path, "lights2000_48x40x2.ppm")
    orc = oracle.OracleScene(rt.parse_gltf_scene(path, 48 / 40))
    fb, st = orc.run_raytracer(48, 40, 2, rng_mode=rt.RT_RNG_REFERENCE)
    assert np.array_equal(oracle.tonemap(fb), ref), f"{int((oracle.tonemap(fb) != ref).any(axis=2).sum())} pixels differ"
    assert deep_walks.inner_plus_lights(orc.bvh_info(1)) == 2555 and st["light_hits"] > 10 * st["light_queries"]  # dozens of terms per sum


def test_live_reference_light_pdf_with_2000_volume_lights_if_present(oracle, rt, sg, tmp_path):
    """bvh_mix_dist::pdf of the reference itself (ref_probe "lightpdf") on 2000 queries of that scene, half of them aimed at lights: the
    oracle's sums of dozens of terms in the same DFS order, bit for bit. The census shows what these queries are."""
    sc = deep_walks.volume_lights_scene(sg, **deep_walks.BIG_LIGHTS)
    path = sg.write_gltf(sc, str(tmp_path / "lights.gltf"))
    rays = deep_walks.light_query_rays(sc, 2000, 77)
    stored = np.load(os.path.join(LIVE, "lights2000_lightpdf.npy"))
    if oracle.have_reference_build():
        rays.astype("<f4").tofile(str(tmp_path / "rays.bin"))
        oracle.ref_probe("lightpdf", path, 48, 40, str(tmp_path / "rays.bin"), str(tmp_path / "lp.bin"))
        assert np.array_equal(np.fromfile(str(tmp_path / "lp.bin"), dtype="<f4").view(np.uint32), stored.view(np.uint32))
    orc = oracle.OracleScene(rt.parse_gltf_scene(path, 48 / 40))
    got = orc.light_pdf(rays)
    assert np.array_equal(got.view(np.uint32), stored.view(np.uint32)), int((got.view(np.uint32) != stored.view(np.uint32)).sum())
    _, light = orc.walk_census(rays)
    deep_walks.require_witnesses("2000 lights, stored light pdf", light, {deep_walks.LIGHT_SHADE_SCRATCH: 0.30})
    assert (stored > 0).mean() > 0.9


def test_live_reference_binary_on_emissive_needles_if_present(oracle, rt, sg, tmp_path):
    """20 000 emissive needles: light queries with up to 14 subtrees pending and closest-hit walks with up to 20. The oracle's PPM is the
    reference binary's."""
    sc = deep_walks.needle_soup_scene(sg, emissive=True, **deep_walks.NEEDLES)
    path = sg.write_gltf(sc, str(tmp_path / "needles.gltf"))
    ref = reference_ppm(oracle, path, 48, 40, 2, tmp_path, "needles20000_48x40x2.ppm")
    orc = oracle.OracleScene(rt.parse_gltf_scene(path, 48 / 40))
    fb, _ = orc.run_raytracer(48, 40, 2, rng_mode=rt.RT_RNG_REFERENCE)
    assert np.array_equal(oracle.tonemap(fb), ref), f"{int((oracle.tonemap(fb) != ref).any(axis=2).sum())} pixels differ"
    closest, light = orc.walk_census(deep_walks.light_query_rays(sc, 2000, 78))
    deep_walks.require_witnesses("emissive needles, light walk", light, {deep_walks.LIGHT_PROBE_SCRATCH: 0.01})
    deep_walks.require_witnesses("emissive needles, closest hit", closest, {deep_walks.CLOSEST_PROBE_SCRATCH: 0.01})


@pytest.mark.parametrize("total", [96, 97])
def test_staging_edge_scenes_have_the_sums_their_names_say(oracle, sg, total):
    """The two light counts tests/test_gpu_deep_walks.py puts on either side of wf_shade's staging rule (inner + lights <= 96), counted on the
    oracle's tree without a GPU."""
    orc = oracle.OracleScene(deep_walks.volume_lights_scene(sg, **deep_walks.STAGING_EDGE[total]))
    assert deep_walks.inner_plus_lights(orc.bvh_info(1)) == total
