"""GPU tests of BVH walks beyond the LDS part of their stacks, device against oracle, bit for bit (scenes and rays: tests/deep_walks.py).

Every traversal stack of the device code has a fast tier in LDS and a slow tier behind it (csrc/rt_dev_stack.h), and the light BVH has two
homes (staged in LDS by wf_shade up to inner + lights = 96, global memory beyond). The other GPU tests stay on one side of each split: at most
40 coplanar lights, at most 3 light references pending, no closest-hit ray shown to hold 14 frames. Each test here first asks the oracle's
census (OracleScene.walk_census) how many deferred siblings its OWN rays keep pending and asserts that enough of them reach the tier it
claims; a render's rays are the ones the oracle logs when it replays the render's pixels (trace_pixel: every ray after a path's first is the
(x, d) of a light query as well). Pending count f and the tier it enters:

    light walk    f >= 5    scratch half of wf_shade's StackMemT<4>            f >= 13   scratch half of the 12-deep stack (probe, megakernel)
    closest hit   f >= 8    first eviction of wf_extend's 6-deep ring          f >= 14   scratch half of the 12-deep stack (probe, megakernel)

Required: 1 % of a test's rays in every tier it claims, 30 % for the light walk's f >= 5. Measured (CPU census; the tests print theirs):

    scene                                      rays                      light f>=5  f>=13  most | closest f>=8  f>=14  most
    2000 volume lights, offsets +-6            20 000 light queries        92.8 %     0      11  |    74.0 %     1.5 %   15
    the same                                   48x40x4 render, replayed   100 %       0      10  |    99.8 %     0       13
    the same                                   2000 wall-to-wall rays     100 %       0      10  |   (64.5 lights hit per query, 98 at most)
    300 volume lights, offsets +-3             20 000 light queries         8.8 %     0       6  |
    20 000 emissive needles                    20 000 light queries        87.5 %    17.2 %  14  |
    the same                                   48x40x2 render, replayed   100 %      23.7 %  14  |   100 %      27.2 %   18
    20 000 needles, 4 ceiling lights           20 000 random + aimed rays                        |    80.9 %    26.3 %   19
    the same                                   48x40x2 render, replayed                          |   100 %      23.5 %   18
"""
import os

import numpy as np
import pytest

import deep_walks as dw
from hit_contract import explain_pixels, summary, verify_hits

pytestmark = pytest.mark.gpu

W, H = 48, 40
COUNTERS = ("samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests",
            "light_tri_tests", "light_hits", "texel_fetches")
ENV_PICTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "envmap", "env.png")
ONE_PERCENT = 0.01


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Case:
    """One scene on the device and in the oracle, with its 20 000 probe rays and everything the oracle says about them, computed once."""

    def __init__(self, gpu, oracle, sc, ray_seed, **build):
        self.sc = sc
        self.dev, self.orc = gpu.DeviceScene(sc, **build), oracle.OracleScene(sc)
        self.rays = dw.light_query_rays(sc, 20000, ray_seed)
        self.closest, self.light = self.orc.walk_census(self.rays)
        self._renders = {}

    def close(self):
        self.dev.close()
        self.orc.close()

    def oracle_render(self, gpu, spp, seed, rng_mode=None):
        """The oracle's framebuffer and counters, and (device-RNG mode) the census of the rays this render casts: closest-hit census of every
        ray, light census of every ray but a path's first."""
        key = (spp, seed, rng_mode)
        if key not in self._renders:
            fb, st = self.orc.run_raytracer(W, H, spp, rng_mode=gpu.RT_RNG_DEVICE if rng_mode is None else rng_mode, seed=seed)
            census = None
            if rng_mode is None:
                rays, later = [], []
                for p in range(0, W * H, 3):  # every third pixel: a third of the render's rays
                    r, smp = self.orc.trace_pixel(W, H, spp, p, seed=seed)
                    rays.append(r)
                    later.append(np.r_[False, smp[1:] == smp[:-1]])
                c, l = self.orc.walk_census(np.concatenate(rays))
                census = (c, l[np.concatenate(later)])
            self._renders[key] = (fb, st, census)
        return self._renders[key]


@pytest.fixture(scope="module")
def big(gpu, oracle, sg):
    c = Case(gpu, oracle, dw.volume_lights_scene(sg, **dw.BIG_LIGHTS), ray_seed=77)
    yield c
    c.close()


@pytest.fixture(scope="module")
def emissive_needles(gpu, oracle, sg):
    c = Case(gpu, oracle, dw.needle_soup_scene(sg, emissive=True, **dw.NEEDLES), ray_seed=78)
    yield c
    c.close()


@pytest.fixture(scope="module")
def needles(gpu, oracle, sg):
    c = Case(gpu, oracle, dw.needle_soup_scene(sg, **dw.NEEDLES), ray_seed=79)
    yield c
    c.close()


def assert_render_is_the_oracles(gpu, case, spp, seed, what, light_tiers, closest_tiers, counters=True, **kw):
    ofb, ost, (c, l) = case.oracle_render(gpu, spp, seed)
    if light_tiers:
        dw.require_witnesses(f"{what}, light queries of the render", l, light_tiers)
    if closest_tiers:
        dw.require_witnesses(f"{what}, casts of the render", c, closest_tiers)
    gfb, gst = case.dev.run_raytracer(W, H, spp, seed=seed, counters=counters, **kw)
    assert np.isfinite(ofb).all()
    assert np.array_equal(bits(gfb), bits(ofb)), f"{what} {kw}: {int((bits(gfb) != bits(ofb)).any(axis=2).sum())} of {W * H} pixels differ from the oracle"
    if counters:
        for k in COUNTERS:
            assert gst[k] == ost[k], f"{what} {kw}: counter {k}: gpu {gst[k]} oracle {ost[k]}"
    return gfb, gst


# ------------------------------------------------------------------------------------------------ the staging rule of wf_shade
EDGE_SCENES = {
    "65_lights_staged": (dict(n_lights=65, size=3.0, seed=7), None, False),
    "sum_96_staged": (dw.STAGING_EDGE[96], 96, False),
    "sum_97_global": (dw.STAGING_EDGE[97], 97, False),
    "300_lights_global_textured": (dict(n_lights=300, size=3.0, seed=8), None, True),
}


@pytest.mark.parametrize("name", list(EDGE_SCENES))
def test_light_tree_on_both_sides_of_the_staging_rule(gpu, oracle, sg, name):
    """wf_shade stages the light tree in LDS when 4 inner + 4 lights <= 384 pieces (light_lds_inner): the last tree that fits (inner + lights
    = 96: the staging copy fills all 384 pieces), the first that does not (97), one well inside and one well outside. Both trees equal the
    oracle's, light_pdf is bit-equal, and a render is the oracle's in every bit and counter with primary rays per lane and in packets."""
    spec, want_sum, textured = EDGE_SCENES[name]
    sc = dw.volume_lights_scene(sg, textured=textured, **spec)
    dev, orc = gpu.DeviceScene(sc), oracle.OracleScene(sc)
    try:
        for which in (0, 1):
            a, b = dev.bvh_info(which), orc.bvh_info(which)
            assert a["root"] == b["root"] and np.array_equal(a["order"], b["order"]) and np.array_equal(a["nodes"], b["nodes"]), which
        total = dw.inner_plus_lights(dev.bvh_info(1))
        print(f"[deep walks] {name}: inner + lights = {total}")
        assert (total == want_sum) if want_sum is not None else ((total <= 96) == name.endswith("staged")), total
        rays = dw.light_query_rays(sc, 20000, 77)
        _, light = orc.walk_census(rays)
        dw.require_witnesses(f"{name}, light queries", light, {dw.LIGHT_SHADE_SCRATCH: ONE_PERCENT} if spec["n_lights"] == 300 else {})
        g, o = dev.light_pdf(rays), orc.light_pdf(rays)
        assert np.array_equal(bits(g), bits(o)), int((bits(g) != bits(o)).sum())
        assert (o > 0).sum() > 1000
        ofb, ost = orc.run_raytracer(W, H, 4, seed=1234)
        for pkt in (gpu.RT_PACKET_OFF, gpu.RT_PACKET_ON):
            gfb, gst = dev.run_raytracer(W, H, 4, seed=1234, counters=True, packet_mode=pkt)
            assert np.array_equal(bits(gfb), bits(ofb)), (name, pkt, int((bits(gfb) != bits(ofb)).any(axis=2).sum()))
            for k in COUNTERS:
                assert gst[k] == ost[k], f"{name}: counter {k}: gpu {gst[k]} oracle {ost[k]} (packet {pkt})"
        plain, _ = dev.run_raytracer(W, H, 4, seed=1234)  # the kernels without counters are other instantiations
        assert np.array_equal(bits(plain), bits(ofb))
        assert ost["light_hits"] > 1000
    finally:
        dev.close()
        orc.close()


# ------------------------------------------------------------------------------------------------ 2000 lights in the volume
def test_big_light_tree_light_pdf(big):
    """light_pdf_kernel on a light tree of 2555 pieces: far beyond anything staged, 11 references pending at most (inside the probe's 12
    LDS positions), so this pins the global tables and long sums; the tier itself is wf_shade's, in the renders below."""
    shares, most = dw.require_witnesses("2000 lights, light queries", big.light, {dw.LIGHT_SHADE_SCRATCH: 0.30})
    assert dw.inner_plus_lights(big.dev.bvh_info(1)) > 2000
    g, o = big.dev.light_pdf(big.rays), big.orc.light_pdf(big.rays)
    assert np.array_equal(bits(g), bits(o)), int((bits(g) != bits(o)).sum())
    assert (o > 0).mean() > 0.9


def test_big_light_tree_render_wavefront_and_megakernel(big, gpu):
    """wf_shade<*, LIGHTS_LDS = false, ENV = false> walking a light tree, most of its queries through the scratch half of its 4-deep stack:
    framebuffer and every event counter are the oracle's, with and without the counting instantiation, and the megakernel agrees."""
    tiers = {dw.LIGHT_SHADE_SCRATCH: 0.30}
    wfb, wst = assert_render_is_the_oracles(gpu, big, 4, 21, "2000 lights, wavefront", tiers, {dw.CLOSEST_RING_EVICT: ONE_PERCENT})
    assert_render_is_the_oracles(gpu, big, 4, 21, "2000 lights, wavefront without counters", None, None, counters=False)
    mfb, mst = assert_render_is_the_oracles(gpu, big, 4, 21, "2000 lights, megakernel", None, None, megakernel=True)
    assert np.array_equal(bits(wfb), bits(mfb))
    for k in COUNTERS:
        assert wst[k] == mst[k], k


def test_big_light_tree_reference_rng(big, gpu):
    """RT_RNG_REFERENCE (one lane per 256-pixel span through the megakernel's 12-deep stack) on the same scene: the oracle's bits."""
    ofb, _, _ = big.oracle_render(gpu, 2, 0, rng_mode=gpu.RT_RNG_REFERENCE)
    gfb, _ = big.dev.run_raytracer(W, H, 2, rng_mode=gpu.RT_RNG_REFERENCE)
    assert np.array_equal(bits(gfb), bits(ofb)), int((bits(gfb) != bits(ofb)).any(axis=2).sum())
    assert np.array_equal(gpu.tonemap(gfb), gpu.tonemap(ofb))


def test_big_light_tree_accumulator(big, gpu):
    """Two rt_accum_render calls of 2 samples are one render of 4 (the accumulator's shade pass is the same wf_shade)."""
    ofb, _, (_, l) = big.oracle_render(gpu, 4, 21)
    dw.require_witnesses("2000 lights, accumulator", l, {dw.LIGHT_SHADE_SCRATCH: 0.30})
    acc = big.dev.accumulator(W, H, seed=21)
    try:
        acc.render(2)
        acc.render(2)
        one, _ = big.dev.run_raytracer(W, H, 4, seed=21)
        assert np.array_equal(bits(acc.image()), bits(one)) and np.array_equal(bits(one), bits(ofb))
    finally:
        acc.close()


def test_big_light_tree_wide_build(big, gpu):
    """The production build (8-wide tree) shades with the same wf_shade: the production contract of tests/test_gpu_production.py. Every pixel
    that differs from the oracle in any bit is explained by a legal hit on one of its paths (an exact tie or a closer hit, the returned
    triangle's own test reproducing it bit for bit), and the image as a whole is the same picture."""
    ofb, ost, (_, l) = big.oracle_render(gpu, 4, 21)
    dw.require_witnesses("2000 lights, wide build", l, {dw.LIGHT_SHADE_SCRATCH: 0.30})
    prod = gpu.DeviceScene(big.sc, wide=True)
    try:
        gfb, gst = prod.run_raytracer(W, H, 4, seed=21, counters=True)
        diff = (bits(gfb) != bits(ofb)).any(axis=2)
        recs = explain_pixels(big.orc, prod, W, H, 4, 21, np.argwhere(diff), "superset", what="2000 lights, wide")
        rel = np.abs(gfb - ofb) / np.maximum(np.abs(ofb), 1e-6)
        bad = (rel > 1e-5).any(axis=2)
        print(f"[deep walks] 2000 lights, wide: {len(recs)} pixels differ in some bit, all explained ({sum(r['cause'] == 'exact tie' for r in recs)} by a tie); "
              f"{int(bad.sum())} of {W * H} beyond 1e-5 relative; casts {gst['casts']} (oracle {ost['casts']})")
        assert bad.mean() <= 0.03, int(bad.sum())
        assert abs(float(gfb.mean()) - float(ofb.mean())) <= 0.02 * float(ofb.mean())
        assert abs(gst["casts"] - ost["casts"]) <= 0.002 * ost["casts"]
    finally:
        prod.close()


def test_big_light_tree_with_environment_map(gpu, oracle, sg):
    """The ENV instantiations of wf_shade read the light tables from global memory whatever their size; until now three lights. The same
    2000 lights in an open room under an environment map: the oracle's framebuffer and counters, wavefront and megakernel."""
    sc = dw.volume_lights_scene(sg, env_texture=gpu.image_decode(ENV_PICTURE), **dw.BIG_LIGHTS)
    case = Case(gpu, oracle, sc, ray_seed=77)
    try:
        assert_render_is_the_oracles(gpu, case, 4, 22, "2000 lights under an environment map", {dw.LIGHT_SHADE_SCRATCH: 0.30}, None)
        assert_render_is_the_oracles(gpu, case, 4, 22, "2000 lights under an environment map, megakernel", None, None, megakernel=True)
        with_map, _, _ = case.oracle_render(gpu, 4, 22)
        sc.bg_texture = -1
        without = oracle.OracleScene(sc)
        nfb, _ = without.run_raytracer(W, H, 4, seed=22)
        without.close()
        assert not np.array_equal(with_map, nfb)  # paths leave the open room: the map is really looked up
    finally:
        case.close()


def test_many_terms_in_one_light_pdf_sum(big, gpu):
    """res += mult / aux.w in DFS order with many terms: rays from one end wall to the other cross the whole volume of lights. Some query
    sums at least 8 lights (counted with the oracle's single-object test of every light), and the sums are the oracle's bits."""
    rays = dw.long_diagonal_rays(big.sc, 2000, seed=9)
    lights = dw.light_triangles(big.sc)
    hits = np.zeros(len(rays), dtype=np.int64)
    for t in lights:
        hit, _ = big.orc.intersect_objects(rays, np.full(len(rays), t, dtype=np.uint32))
        hits += hit
    _, light = big.orc.walk_census(rays)
    dw.require_witnesses("2000 lights, end-to-end rays", light, {dw.LIGHT_SHADE_SCRATCH: 0.30})
    print(f"[deep walks] lights hit by one query: most {int(hits.max())}, mean {hits.mean():.1f}; {int((hits >= 8).sum())} of {len(rays)} queries sum >= 8 terms")
    assert hits.max() >= 8 and (hits >= 8).mean() >= ONE_PERCENT
    g, o = big.dev.light_pdf(rays), big.orc.light_pdf(rays)
    assert np.array_equal(bits(g), bits(o)), int((bits(g) != bits(o)).sum())
    assert np.isfinite(o[hits >= 8]).all() and (o[hits >= 8] > 0).all()


# ------------------------------------------------------------------------------------------------ 20 000 emissive needles: the deep light walk
def test_deep_light_walk_light_pdf(emissive_needles):
    """light_pdf_kernel beyond the 12 LDS positions of its stack (push_ref / pop_ref with sp >= 12)."""
    c = emissive_needles
    dw.require_witnesses("emissive needles, light queries", c.light, {dw.LIGHT_SHADE_SCRATCH: 0.30, dw.LIGHT_PROBE_SCRATCH: ONE_PERCENT})
    g, o = c.dev.light_pdf(c.rays), c.orc.light_pdf(c.rays)
    assert np.array_equal(bits(g), bits(o)), int((bits(g) != bits(o)).sum())
    assert (o > 0).sum() > 1000


def test_deep_light_walk_renders(emissive_needles, gpu):
    """The same tree under both renderers: the megakernel's light walk beyond its 12 LDS positions, wf_shade's beyond its 4."""
    c = emissive_needles
    assert_render_is_the_oracles(gpu, c, 2, 5, "emissive needles, megakernel", {dw.LIGHT_PROBE_SCRATCH: ONE_PERCENT}, {dw.CLOSEST_PROBE_SCRATCH: ONE_PERCENT},
                                 megakernel=True)
    assert_render_is_the_oracles(gpu, c, 2, 5, "emissive needles, wavefront", {dw.LIGHT_SHADE_SCRATCH: 0.30}, {dw.CLOSEST_RING_EVICT: ONE_PERCENT})


# ------------------------------------------------------------------------------------------------ 20 000 needles: the deep closest-hit walk
@pytest.fixture(scope="module")
def needle_hits(needles):
    return needles.orc.cast_rays(needles.rays)


def test_deep_closest_hit_probe(needles, needle_hits):
    """cast_kernel beyond the 12 LDS positions of its stack (the newest frame is in registers: 14 pending frames and more)."""
    dw.require_witnesses("needles, probe rays", needles.closest, {dw.CLOSEST_PROBE_SCRATCH: ONE_PERCENT})
    op, ob = needle_hits
    gp, gb = needles.dev.cast_rays(needles.rays)
    assert np.array_equal(gp, op), f"{int((gp != op).sum())} hit-index mismatches"
    assert np.array_equal(bits(gb), bits(ob)), "b/c/t differ in bits"
    assert (op != 0xFFFFFFFF).sum() > 1000  # (needles poke through the walls, and so do some ray origins)


def test_deep_closest_hit_wavefront_kernels(needles, needle_hits, gpu):
    """wf_extend and wf_extend_packet with their ring evicting to the global workspace and refilling from it: the oracle's hits, and the two
    kernels count the same visits. The global-best variants (2-word frames) under their contract: hit / miss and t bit-equal, an index may
    differ only as an exact tie that the returned triangle's own test reproduces."""
    dw.require_witnesses("needles, probe rays", needles.closest, {dw.CLOSEST_RING_EVICT: ONE_PERCENT, dw.CLOSEST_PROBE_SCRATCH: ONE_PERCENT})
    op, ob = needle_hits
    rays = needles.rays
    stats = {}
    for mode in (gpu.RT_CAST_EXTEND, gpu.RT_CAST_PACKET):
        gp, gb, stats[mode] = needles.dev.cast_rays_ex(rays, mode)
        assert np.array_equal(gp, op), (mode, int((gp != op).sum()))
        assert np.array_equal(bits(gb), bits(ob)), mode
    for k in ("nodes_visited", "box_tests", "tri_tests"):
        assert stats[gpu.RT_CAST_EXTEND][k] == stats[gpu.RT_CAST_PACKET][k], (k, stats[gpu.RT_CAST_EXTEND][k], stats[gpu.RT_CAST_PACKET][k])
    for mode in (gpu.RT_CAST_EXTEND_GLOBAL, gpu.RT_CAST_PACKET_GLOBAL):
        gp, gb, st = needles.dev.cast_rays_ex(rays, mode)
        c = verify_hits(needles.orc, rays, op, ob, gp, gb, "exact", brute=1024, what=f"needles, mode {mode}")
        print(f"[deep walks] needles, mode {mode}: {summary(c)}")
        assert st["nodes_visited"] <= stats[gpu.RT_CAST_EXTEND]["nodes_visited"]


def test_deep_closest_hit_wide_build(needles, needle_hits, gpu):
    """The 8-wide tree of the same soup under the superset contract: t is the brute-force minimum, never farther than the oracle's, and every
    hit that differs from the oracle's is the returned triangle's own hit bit for bit."""
    op, ob = needle_hits
    prod = gpu.DeviceScene(needles.sc, wide=True)
    try:
        for mode in (gpu.RT_CAST_EXTEND, gpu.RT_CAST_PACKET):
            gp, gb, st = prod.cast_rays_ex(needles.rays, mode)
            c = verify_hits(needles.orc, needles.rays, op, ob, gp, gb, "superset", brute=1024, what=f"needles, wide, mode {mode}")
            print(f"[deep walks] needles, wide, mode {mode}: {summary(c)}")
            assert st["nodes_visited"] > 0
    finally:
        prod.close()


def test_deep_closest_hit_renders(needles, gpu):
    """A render whose casts go that deep: the megakernel beyond its 12 LDS positions, the wavefront pipeline with ring evictions."""
    assert_render_is_the_oracles(gpu, needles, 2, 6, "needles, megakernel", None, {dw.CLOSEST_PROBE_SCRATCH: ONE_PERCENT}, megakernel=True)
    assert_render_is_the_oracles(gpu, needles, 2, 6, "needles, wavefront", None, {dw.CLOSEST_RING_EVICT: ONE_PERCENT})
