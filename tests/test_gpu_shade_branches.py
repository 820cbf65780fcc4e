"""The shading path of the HIP kernels (make_surf, TexFoot::fetch, tex_sample, tex_sample_set, shade_hit: csrc/rt_dev_surface.h,
csrc/rt_dev_shade.h) against the oracle, bit for bit, on the fixtures of tests/shade_branches.py: scenes and rays built to take every branch.

Every test first asserts, from the oracle's shade census, that its rays take every slot the fixture claims (the same assertion as
tests/test_shade_census.py makes on the CPU), and only then compares:
  * rt_render_rays with OracleScene.trace_rays and its fold, event counters included, on rays no camera makes;
  * the same radiance through RT_FLAG_GLOBAL_BEST, the wide tree, the device-built wide tree, and split into passes under every sort / packet mode;
  * camera renders through the wavefront pipeline, the megakernel and the reference RNG (shade_hit's other instantiation);
  * a feature accumulator (wf_features runs the same make_surf) and the device film.
All comparisons are on uint32 views."""
import importlib
import os

import numpy as np
import pytest

import feature_replay as fr
import shade_branches as sb

pytestmark = pytest.mark.gpu

COUNTERS = ("samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests",
            "light_tri_tests", "light_hits", "texel_fetches")
K, SEED = sb.SAMPLES, sb.SEED
W, H, SPP = sb.CAMERA


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_bits(got, want, what):
    fr.assert_bits(np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32), what)


@pytest.fixture(scope="module")
def abi():
    return importlib.import_module("raytracing-course-hw-public_amd._ctypes_abi")


@pytest.fixture(scope="module")
def case(gpu, oracle, sg):
    """name -> the fixture, its oracle scene, the census of its caller rays (asserted against its claims), and the oracle's per-sample radiance of
    the packings the tests use. Computed once per fixture and shared; nobody writes to them."""
    cache = {}

    def get(name):
        if name not in cache:
            sc, rays, claimed = sb.make(name, sg, gpu)
            orc = oracle.OracleScene(sc)
            sb.require(f"{name}, caller rays", orc.shade_census(rays, K, seed=SEED), claimed)
            c = dict(sc=sc, rays=rays, claimed=claimed, orc=orc, packed={}, per={}, stats={})
            for (k, g) in ((1, 1), (K, 1), (K, 4)):
                c["packed"][k, g] = gpu.pack_rays(rays, samples=k, rays_per_output=g)
                c["per"][k, g], c["stats"][k, g] = orc.trace_rays(c["packed"][k, g], k, seed=SEED)
                c["per"][k, g].setflags(write=False)
            cache[name] = c
        return cache[name]

    return get


@pytest.mark.parametrize("name", sb.FIXTURES)
def test_render_rays_equal_the_oracle(gpu, oracle, case, name):
    c = case(name)
    dev = gpu.DeviceScene(c["sc"])
    for (k, g) in ((1, 1), (K, 1), (K, 4)):
        out, st = dev.render_rays(c["packed"][k, g], samples=k, rays_per_output=g, seed=SEED, counters=True)
        per = c["per"][k, g]
        if (k, g) == (1, 1):
            _assert_bits(out, per[:, 0], f"{name}: K = 1, G = 1 against trace_rays")  # the samples themselves, no fold
        _assert_bits(out, oracle.fold_outputs(per, g), f"{name}: K = {k}, G = {g} against the fold of trace_rays")
        for key in COUNTERS:
            assert st[key] == c["stats"][k, g][key], (name, k, g, key, st[key], c["stats"][k, g][key])
        assert np.count_nonzero(np.any(out != 0, axis=1)) * 2 >= len(out)
    dev.close()


@pytest.mark.parametrize("name", sb.FIXTURES)
def test_other_tree_kinds_and_pass_splits_change_no_bit(gpu, oracle, case, name):
    """No two triangles of a fixture are coplanar and overlapping, so every traversal finds the same closest hit and the radiance is the
    oracle's on every tree. Counters are not compared: other trees visit other nodes."""
    c = case(name)
    want = oracle.fold_outputs(c["per"][K, 1], 1)
    rays = c["packed"][K, 1]
    parity = gpu.DeviceScene(c["sc"])
    out, _ = parity.render_rays(rays, samples=K, seed=SEED, global_best=True)
    _assert_bits(out, want, f"{name}: RT_FLAG_GLOBAL_BEST")
    assert len(rays) > 1024
    for sort in (gpu.RT_SORT_OFF, gpu.RT_SORT_OCTANT_CELL_CONE):
        for packet in (gpu.RT_PACKET_OFF, gpu.RT_PACKET_ON):
            out, st = parity.render_rays(rays, samples=K, seed=SEED, max_paths=1024, sort_mode=sort, packet_mode=packet)
            assert st["passes"] >= 2 * K, (name, st["passes"])  # more than 1024 outputs: several output tiles, a pass per tile and sample
            _assert_bits(out, want, f"{name}: max_paths 1024, sort {sort}, packet {packet}")
    parity.close()
    for kw in (dict(wide=True), dict(wide=True, device_bvh=True)):
        dev = gpu.DeviceScene(c["sc"], **kw)
        out, _ = dev.render_rays(rays, samples=K, seed=SEED)
        _assert_bits(out, want, f"{name}: {kw}")
        dev.close()


@pytest.mark.parametrize("name", sb.FIXTURES)
def test_camera_renders_equal_the_oracle(gpu, oracle, case, name):
    c = case(name)
    orc = c["orc"]
    cam_claimed = [s for s in c["claimed"] if s not in sb.CAMERA_UNCLAIMED]
    dev = gpu.DeviceScene(c["sc"])
    for what, rng_mode, kw in (("wavefront", gpu.RT_RNG_DEVICE, {}), ("megakernel", gpu.RT_RNG_DEVICE, dict(megakernel=True)),
                               ("reference RNG", gpu.RT_RNG_REFERENCE, {})):
        sb.require(f"{name}, camera, {what}", orc.shade_census_render(W, H, SPP, seed=SEED, rng_mode=rng_mode), cam_claimed)
        want, ost = orc.run_raytracer(W, H, SPP, rng_mode=rng_mode, seed=SEED)
        fb, st = dev.run_raytracer(W, H, SPP, rng_mode=rng_mode, seed=SEED, counters=True, **kw)
        _assert_bits(fb, want, f"{name}: camera render, {what}")
        for key in COUNTERS:
            assert st[key] == ost[key], (name, what, key, st[key], ost[key])
    dev.close()


def test_ray_kinds_equal_the_oracle(gpu, oracle, sg, abi):
    """Unnormalised, axis-parallel and plane-parallel directions, origins on and inside surfaces, streams and sample indices at 0, 2^31 and
    2^32 - 1 (K = 3 wraps the index), every rays_per_output with every K."""
    sc, packed, claimed = sb.ray_kinds(sg, gpu, abi)
    orc = oracle.OracleScene(sc)
    dev = gpu.DeviceScene(sc)
    wide = gpu.DeviceScene(sc, wide=True, device_bvh=True)
    for k in sb.RAY_KIND_SAMPLES:
        sb.require(f"ray_kinds, K = {k}", orc.shade_census(packed, k, seed=SEED), claimed)
        per, ost = orc.trace_rays(packed, k, seed=SEED)
        for g in sb.RAY_KIND_OUTPUTS:
            out, st = dev.render_rays(packed, samples=k, rays_per_output=g, seed=SEED, counters=True)
            _assert_bits(out, oracle.fold_outputs(per, g), f"ray_kinds: K = {k}, G = {g}")
            for key in COUNTERS:
                assert st[key] == ost[key], (k, g, key, st[key], ost[key])
        out, _ = wide.render_rays(packed, samples=k, rays_per_output=4, seed=SEED)
        _assert_bits(out, oracle.fold_outputs(per, 4), f"ray_kinds on the wide tree: K = {k}")
    dev.close()
    wide.close()


def test_device_film_on_tex_edges(gpu, oracle, case):
    c = case("tex_edges")
    dev = gpu.DeviceScene(c["sc"])
    out8, _ = dev.render_rays(c["packed"][K, 4], samples=K, rays_per_output=4, seed=SEED, rgb8=True)
    want = oracle.tonemap(oracle.fold_outputs(c["per"][K, 4], 4))
    assert out8.dtype == np.uint8 and np.array_equal(out8, want)
    assert len(np.unique(out8.reshape(-1, 3), axis=0)) > 100  # texels, not a flat colour
    dev.close()


@pytest.mark.parametrize("name", ["tex_edges", "surf_edges"])
def test_feature_accumulator(gpu, oracle, case, name):
    """wf_features runs make_surf on the primary hits. Hits and depth against the oracle's closest hits; the albedo against the oracle's samples
    of the twin scene (feature_replay: emission := colour, depth 1) on tex_edges, whose colour maps are read at every footprint kind, and
    against the hit triangle's material colour on surf_edges, which has no colour map (its NaN normals would turn the twin's sample into
    0 x NaN); the normal sum against the surface-normal probe, another kernel over the same make_surf: NaN where it is NaN (zero tangents,
    zero normals), the same bits elsewhere."""
    c = case(name)
    sc, orc = c["sc"], c["orc"]
    dev = gpu.DeviceScene(sc)
    n = SPP
    rays = fr.primary_rays(orc, W, H, n, SEED)
    hit, t, prim = fr.first_hits(orc, rays)
    assert hit.sum() * 4 >= hit.size
    if name == "tex_edges":
        assert fr.twin_alpha_is_one(sc)
        tw = oracle.OracleScene(fr.twin_scene(sc))
        albedo = tw.pixel_samples(W, H, n, np.arange(W * H), seed=SEED)
        # the colour lookups of the primary hits take the footprints the fixture is about
        cen = tw.shade_census_render(W, H, n, seed=SEED)
        sb.require(f"{name}, twin", cen, [f"{k}_gamma" for k in sb.TEX_KINDS])
    else:
        assert all(m.color_tex < 0 for m in sc.materials)
        colors = np.array([m.color[:3] for m in sc.materials], np.float32)
        albedo = np.where(hit[..., None], colors[sc.material_ids[np.where(hit, prim, 0)]], np.float32(0))
    _, _, _, sn = dev.surface_normals(rays.reshape(-1, 6))
    sn = sn.reshape(W * H, n, 3)
    acc = dev.accumulator(W, H, seed=SEED, features=True)
    acc.render(1)
    acc.render(n - 1)
    f = acc.read_features()
    assert np.all(acc.read()["samples"] == n)
    assert np.array_equal(f["hits"], fr.hit_ladder(hit)[n].reshape(H, W))
    fr.assert_bits(f["depth_sum"], fr.ladder(t)[n].reshape(H, W), f"{name}: ZS")
    fr.assert_bits(f["albedo_sum"], fr.ladder(albedo)[n].reshape(H, W, 3), f"{name}: AS")
    want_n = fr.ladder(sn)[n].reshape(H, W, 3)
    nan = np.isnan(want_n)
    assert np.array_equal(np.isnan(f["normal_sum"]), nan)
    assert nan.any() == (name == "surf_edges")
    fr.assert_bits(np.where(nan, np.float32(0), f["normal_sum"]), np.where(nan, np.float32(0), want_n), f"{name}: NS")
    acc.close()
    dev.close()


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shade_branches")


@pytest.mark.parametrize("name", ["tex_edges_safe", "surf_edges", "brdf_edges_three_lights", "brdf_edges_many_lights"])
def test_reference_rng_render_is_the_unmodified_references(gpu, oracle, sg, tmp_path, name):
    """The HIP path against the stored renders of the unmodified reference binary on the fixtures' scenes, as far as glTF carries them
    (shade_branches.reference_scenes says what is lost; tests/test_shade_census.py holds the oracle to the same files without a GPU): the
    film of the reference-RNG render, on the device and on the host, byte for byte."""
    w, h, spp = sb.REFERENCE_RENDER
    path = sg.write_gltf(sb.reference_scenes(sg, gpu)[name], str(tmp_path / (name + ".gltf")))
    stored = oracle.read_ppm(os.path.join(GOLDEN, sb.reference_ppm_name(name)))
    ls = gpu.parse_gltf_scene(path, w / h)
    sb.require(f"{name}, reference render", oracle.OracleScene(ls).shade_census_render(w, h, spp, rng_mode=gpu.RT_RNG_REFERENCE), sb.REFERENCE_CLAIMS[name])
    dev = gpu.DeviceScene(ls)
    img, _ = dev.run_raytracer_rgb8(w, h, spp, rng_mode=gpu.RT_RNG_REFERENCE)
    assert np.array_equal(img, stored), f"{name}: {int((img != stored).any(axis=2).sum())} pixels differ (device film)"
    fb, _ = dev.run_raytracer(w, h, spp, rng_mode=gpu.RT_RNG_REFERENCE)
    assert np.array_equal(gpu.tonemap(fb), stored), name
    dev.close()
