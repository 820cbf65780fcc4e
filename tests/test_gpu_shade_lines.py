"""wf_shade's texture lookups through footprint records (csrc/rt_tex_views.h, rt_dev_surface.h tex_sample_set) and the split fold frames
(rt_device_types.h WfFold: a scale record always, an emission record only where the emission is not exactly +0), against the oracle.

Both changes move bytes, not values: every image and every event counter must be the oracle's bit for bit, in both texture layouts
(RT_BUILD_TEX_TILED forces the interleaved tiles), on the parity tree, with global-best pruning and on the wide tree. For the two production
traversals the counters compared are the ones a traversal cannot change (samples, casts, shaded hits, texel fetches, the light queries):
their node, box and triangle counts count another tree or another pruning rule by design ("Two kinds of modes")."""
import numpy as np
import pytest

import adaptive_replay as ar
from conftest import random_rays

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 48, 32, 4, 11
ALL = ("samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests", "light_tri_tests", "light_hits",
       "texel_fetches")
PATHS_ONLY = ("samples", "casts", "shaded_hits", "light_queries", "texel_fetches")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _tex(rng, w, h):
    t = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    t[..., 3] = 255
    return t


def _texture_scene(sg):
    """About 300 triangles; four texture sets (colour, normal, metallic-roughness, and an emissive map on two of them) of 5x3, 8x8, 1x1 and
    33x17 texels: no multiple of the 4 x 2 tile, exactly tiles, the 1x1 fast path (never interleaved), several tiles with a ragged edge.
    Texcoords run over [-3, 3]: negatives, values >= 1, and the exact grid, integer and rounds-up-to-1.0f cases of TexFoot."""
    rng = np.random.default_rng(5)
    sc = sg.room_scene(288, seed=23, n_lights=3, n_materials=8, tex_size=0, alpha_fraction=0.0)
    sc.ray_depth = 5
    sc.textures = []
    for k, (w, h) in enumerate(((5, 3), (8, 8), (1, 1), (33, 17))):
        sc.textures += [_tex(rng, w, h) for _ in range(4)]
        for m in sc.materials[2 + 2 * k: 4 + 2 * k]:
            m.color_tex, m.normal_tex, m.metallic_roughness_tex = 4 * k, 4 * k + 1, 4 * k + 2
        sc.materials[2 + 2 * k].emissive_tex = 4 * k + 3
        sc.materials[2 + 2 * k].emission = (0.25, 0.125, 0.5)
    sc.texcoords = rng.uniform(-3, 3, size=sc.texcoords.shape).astype(np.float32)
    sc.texcoords[:40] = rng.integers(-3, 4, size=(40, 3, 2)).astype(np.float32) / np.float32(5)
    sc.texcoords[40:60] = np.float32(-1e-9)
    return sc


def _emission_scene(sg):
    """Materials whose emission words are +0, -0.0, a denormal and inf, three of them behind an emissive map (whose zero texels turn inf into
    NaN and leave -0.0 a -0.0): frames with and without an emission record, and every bit pattern the flag must not mistake for +0."""
    rng = np.random.default_rng(6)
    sc = sg.room_scene(288, seed=29, n_lights=2, n_materials=8, tex_size=0, alpha_fraction=0.0)
    sc.ray_depth = 5
    em = _tex(rng, 8, 8)
    em[::2, ::3, :3] = 0
    sc.textures = [em]
    emissions = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (0.0, -0.0, -0.0), (0.0, 1e-40, 0.0), (0.0, 0.0, float("inf")), (1e-42, 0.0, 0.0)]
    for i, (m, e) in enumerate(zip(sc.materials[2:], emissions)):
        m.emission = e
        if i in (1, 4, 6):
            m.emissive_tex = 0
    sc.materials[0].emission = (0.0, 0.0, 0.0)  # the walls: most frames have no emission record
    sc.texcoords = rng.uniform(-2, 2, size=sc.texcoords.shape).astype(np.float32)
    return sc


@pytest.fixture(scope="module")
def textured(gpu, oracle, sg):
    """The first scene, its oracle image and counters, computed once; nobody writes to them."""
    sc = _texture_scene(sg)
    orc = oracle.OracleScene(sc)
    fb, st = orc.run_raytracer(W, H, SPP, seed=SEED)
    fb.setflags(write=False)
    yield sc, orc, fb, st
    orc.close()


@pytest.mark.parametrize("tiled", [False, True], ids=["footprint", "tiled"])
@pytest.mark.parametrize("build", ["parity", "global_best", "wide", "wide_device"])
def test_image_and_counters_are_the_oracles(gpu, textured, build, tiled):
    sc, _, ofb, ost = textured
    kw = {"parity": {}, "global_best": {}, "wide": dict(wide=True), "wide_device": dict(wide=True, device_bvh=True)}[build]
    dev = gpu.DeviceScene(sc, build_flags=gpu.RT_BUILD_TEX_TILED if tiled else 0, **kw)
    try:
        fb, st = dev.run_raytracer(W, H, SPP, seed=SEED, counters=True, global_best=build == "global_best")
        print(build, "tiled" if tiled else "footprint", {k: st[k] for k in ALL})
        assert np.array_equal(_bits(fb), _bits(ofb)), (build, tiled, int((_bits(fb) != _bits(ofb)).any(axis=2).sum()))
        for k in ALL if build == "parity" else PATHS_ONLY:
            assert st[k] == ost[k], (build, tiled, k, st[k], ost[k])
        assert st["texel_fetches"] > 0
        if build == "parity":  # the megakernel samples through the same records
            mfb, mst = dev.run_raytracer(W, H, SPP, seed=SEED, counters=True, megakernel=True)
            assert np.array_equal(_bits(mfb), _bits(ofb)) and mst["texel_fetches"] == ost["texel_fetches"]
    finally:
        dev.close()


def test_footprint_and_tiled_layouts_agree(gpu, textured):
    """The two layouts of one library against each other: image, counters, and the closest hits."""
    sc = textured[0]
    a, b = gpu.DeviceScene(sc), gpu.DeviceScene(sc, build_flags=gpu.RT_BUILD_TEX_TILED)
    try:
        fa, sa = a.run_raytracer(W, H, SPP, seed=SEED + 1, counters=True)
        fb, sb = b.run_raytracer(W, H, SPP, seed=SEED + 1, counters=True)
        assert np.array_equal(_bits(fa), _bits(fb))
        for k in ALL:
            assert sa[k] == sb[k], k
    finally:
        a.close()
        b.close()


def test_every_pass_kind_folds_the_split_frames(gpu, oracle, textured):
    """An accumulator pass and a rt_render_rays call on the first scene: the passes whose first and last stages are not rt_render's."""
    sc, orc, ofb, _ = textured
    dev = gpu.DeviceScene(sc)
    try:
        acc = dev.accumulator(W, H, seed=SEED)
        acc.render(SPP)
        x = orc.pixel_samples(W, H, SPP, np.arange(W * H), seed=SEED).reshape(H, W, SPP, 3)
        ar.assert_state(acc.read(), *ar.fold(x), np.full((H, W), SPP), what="accumulator pass")
        assert np.array_equal(_bits(acc.image()), _bits(ofb))
        acc.close()
        rays = random_rays(sc, 1500, seed=3)
        out, st = dev.render_rays(rays, samples=2, seed=SEED, counters=True)
        per, rst = orc.trace_rays(rays, 2, seed=SEED)
        assert np.array_equal(_bits(out), _bits(oracle.fold_outputs(per, 1)))
        for k in ALL:
            assert st[k] == rst[k], k
    finally:
        dev.close()


def test_frames_with_and_without_emission(gpu, oracle, sg):
    """Emission words 0, -0.0, a denormal and inf, some behind an emissive map: image and counters are the oracle's, so wf_fold read every stored
    emission and implied only exact +0. That both branches ran follows from counts: of the pushed frames (the oracle's census of this very
    render) at most `lit` belong to a hit on a material whose emission has a non-zero bit and at most `unlit` to one without, so at least
    pushed - lit frames had no emission record and at least pushed - unlit had one."""
    sc = _emission_scene(sg)
    orc = oracle.OracleScene(sc)
    dev = gpu.DeviceScene(sc)
    try:
        ofb, ost = orc.run_raytracer(W, H, SPP, seed=SEED)
        for kw in ({}, {"global_best": True}, {"megakernel": True}):
            fb, st = dev.run_raytracer(W, H, SPP, seed=SEED, counters=True, **kw)
            assert np.array_equal(_bits(fb), _bits(ofb)), kw
            for k in PATHS_ONLY if kw.get("global_best") else ALL:
                assert st[k] == ost[k], (kw, k)
        assert np.isinf(ofb).any() and np.isfinite(ofb).any()
        pushed = orc.shade_census_render(W, H, SPP, seed=SEED)["shade_push"]
        rays = np.concatenate([orc.trace_pixel(W, H, SPP, p, seed=SEED)[0] for p in range(W * H)])
        assert len(rays) == ost["casts"]
        prim, _ = orc.cast_rays(rays)
        hit = prim != 0xFFFFFFFF
        assert int(hit.sum()) == ost["shaded_hits"] == st["shaded_hits"]
        bits_set = np.array([bool(np.any(_bits(m.emission_f32()) != 0)) for m in sc.materials])
        lit_hit = bits_set[sc.material_ids[prim[hit]]]
        lit, unlit = int(lit_hit.sum()), int((~lit_hit).sum())
        print(f"frames pushed {pushed}; hits on materials with emission bits {lit}, without {unlit}")
        assert pushed - lit > 0 and pushed - unlit > 0
    finally:
        dev.close()
        orc.close()
