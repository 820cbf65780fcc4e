"""Production traversal modes against the CPU oracle.

The parity mode reproduces the reference's traversal exactly (bvh.h:195-235: near-local pruning, reference topology) and is
pinned elsewhere bit for bit. The production modes do LESS work than the reference:
  * RT_FLAG_GLOBAL_BEST / RT_CAST_*_GLOBAL : every box is culled against the global best hit so far;
  * RT_BUILD_WIDE                          : 8-wide nodes with quantised child boxes (tests further below, when built).
Their contract is checked against the ORACLE (never against another GPU scene): the closest hit's `t` must be bit-equal on
every ray; hit indices may differ only where two triangles share that exact `t` (a tie the reference resolves by its own
traversal order); the mismatch count is asserted, not printed. The event counters must show the mode really visits fewer nodes.
(One refinement for binary production trees on overlapping coplanar triangles, where the reference's own pruning rule lets the tree shape pick between
two hits an ulp apart: test_overlapping_coplanar_triangles_and_the_binary_production_trees.)
On top of the counts, every hit that differs from the oracle's is checked exactly (tests/hit_contract.py): the oracle's single-object test of the
returned index reproduces it bit for bit, and no hit lies below the brute-force minimum — the wide tree's t IS that minimum. Every pixel of a
production render that differs from the oracle (or the parity image) in any bit is explained by such a hit on one of its paths (explain_pixels).
"""
import numpy as np
import pytest

import hit_contract
from conftest import random_rays
from guarded_rays import big_leaf_scene, degenerate_rays, fast_division_boundary_rays, is_guarded
from hit_contract import explain_pixels, summary, verify_hits, verify_reported_hits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report_hit_contract_time():
    t0 = hit_contract.STATS["seconds"]
    yield
    print(f"\n[hit contract] {hit_contract.STATS['seconds'] - t0:.1f} s of this module's run spent in verify_hits / explain_pixels")


FIXTURES = ["room_plain", "room_textured", "open_nolight", "boxes", "room_manylights"]


def compare_hits_with_oracle(orc, rays, op, ob, gp, gb, what, brute="all"):
    """`t` bit-equal on every ray; an index mismatch is legal only as an exact tie (same t bits, both hit), verified bit for bit by the oracle's
    test of the returned triangle (hit_contract.verify_hits, kind "exact"). Returns the tie count."""
    ot, gt = ob[:, 2].view(np.uint32), gb[:, 2].view(np.uint32)
    miss_o, miss_g = op == 0xFFFFFFFF, gp == 0xFFFFFFFF
    assert np.array_equal(miss_o, miss_g), f"{what}: {int((miss_o != miss_g).sum())} rays hit on one side only"
    bad_t = ot != gt
    assert not bad_t.any(), f"{what}: t differs from the oracle on {int(bad_t.sum())} of {len(op)} rays (first: ray {int(np.flatnonzero(bad_t)[0])})"
    ties = (op != gp) & ~miss_o
    # where the index agrees, the barycentrics are the same triangle test on the same operands: bit-equal too
    same = ~ties
    assert np.array_equal(gb[same].view(np.uint32), ob[same].view(np.uint32)), f"{what}: b/c differ on rays with the oracle's own triangle"
    c = verify_hits(orc, rays, op, ob, gp, gb, "exact", brute=brute, what=what)
    print(f"{what}: {summary(c)}")
    assert c["ties"] == int(ties.sum())
    return int(ties.sum())


def compare_superset_hits_with_oracle(orc, rays, op, ob, gp, gb, what, max_rel=1e-6, brute="all", kind="superset"):
    """The wide traversal tests conservative SUPERSETS of the reference's boxes and culls against the global best, so it can
    only find what the reference finds, or something CLOSER that the reference's own pruning skipped: bvh.h:216-223 prunes a far
    child whose rounded slab-entry distance is >= the near hit, although a triangle inside may round to a smaller t (flat boxes
    of axis-aligned triangles; SURVEY 7 names the case). Asserts: never a farther hit, never a miss where the reference hits;
    closer hits are rounding-sized (<= max_rel relative); and exactly (hit_contract.verify_hits, kind "superset"): every differing hit is the
    returned object's own hit bit for bit, and t is the brute-force minimum. Returns (exact ties resolved to another index, closer hits)."""
    miss_o, miss_g = op == 0xFFFFFFFF, gp == 0xFFFFFFFF
    assert not (miss_g & ~miss_o).any(), f"{what}: {int((miss_g & ~miss_o).sum())} rays miss although the reference hits"
    both = ~miss_o & ~miss_g
    ot, gt = ob[:, 2], gb[:, 2]
    assert not (both & (gt > ot)).any(), f"{what}: {int((both & (gt > ot)).sum())} rays return a FARTHER hit than the reference"
    closer = (both & (gt < ot)) | (miss_o & ~miss_g)
    rel = (ot[both] - gt[both]) / np.maximum(ot[both], 1e-30)
    assert rel.max(initial=0.0) <= max_rel, f"{what}: a hit is closer than the reference's by {float(rel.max()):.3e} relative: more than rounding"
    assert not (miss_o & ~miss_g).any() or max_rel > 1e-3, f"{what}: {int((miss_o & ~miss_g).sum())} rays hit although the reference misses"
    ties = both & (gt == ot) & (op != gp)
    same = both & (op == gp)
    assert np.array_equal(gb[same].view(np.uint32), ob[same].view(np.uint32)), f"{what}: (b, c, t) differ on a ray with the oracle's own triangle"
    c = verify_hits(orc, rays, op, ob, gp, gb, kind, brute=brute, what=what)
    print(f"{what}: {summary(c)}")
    assert c["ties"] == int(ties.sum()) and c["closer"] + c["oracle_miss"] == int(closer.sum())
    return int(ties.sum()), int(closer.sum())


@pytest.fixture(scope="module")
def pairs(gpu, oracle, scenes):
    out = {}
    for name, sc in scenes.items():
        out[name] = (gpu.DeviceScene(sc), oracle.OracleScene(sc), sc)
    yield out
    for d, o, _ in out.values():
        d.close()
        o.close()


def _camera_rays(sc, n, seed):
    """Rays from the camera position (what primary rays look like: one origin, a packet-friendly fan of directions)."""
    rng = np.random.default_rng(seed)
    cam = sc.camera
    f, r, u = np.asarray(cam.forward, np.float32), np.asarray(cam.right, np.float32), np.asarray(cam.up, np.float32)
    a = rng.uniform(-0.5, 0.5, size=(n, 2)).astype(np.float32)
    a = a[np.lexsort((a[:, 0], np.floor(a[:, 1] * 64)))]  # scanline-ish order: 64 consecutive rays are neighbours
    d = f[None, :] + a[:, :1] * r[None, :] + a[:, 1:] * u[None, :]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.tile(np.asarray(cam.position, np.float32), (n, 1))
    return np.concatenate([o, d.astype(np.float32)], axis=1).astype(np.float32)


@pytest.mark.parametrize("name", FIXTURES)
def test_wavefront_probe_in_parity_mode_is_the_oracle(pairs, gpu, name):
    """rt_cast_rays_ex through wf_extend / wf_extend_packet in the reference's traversal order: every field bit-equal, and
    the kernels' event counters equal the per-lane probe's semantics (nodes and triangle tests are the oracle's)."""
    dev, orc, sc = pairs[name]
    rays = np.concatenate([random_rays(sc, 6000, seed=7), _camera_rays(sc, 4096 + 37, seed=8)])
    op, ob = orc.cast_rays(rays)
    for mode in (gpu.RT_CAST_EXTEND, gpu.RT_CAST_PACKET):
        gp, gb, st = dev.cast_rays_ex(rays, mode)
        assert np.array_equal(gp, op), (name, mode, int((gp != op).sum()))
        assert np.array_equal(gb.view(np.uint32), ob.view(np.uint32)), (name, mode)
        assert st["casts"] == len(rays) and st["nodes_visited"] > 0


@pytest.mark.parametrize("name", FIXTURES)
def test_global_best_hits_equal_the_oracle(pairs, gpu, name):
    dev, orc, sc = pairs[name]
    rays = np.concatenate([random_rays(sc, 20000, seed=101), _camera_rays(sc, 8192, seed=102)])
    op, ob = orc.cast_rays(rays)
    _, _, st_ref = dev.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
    for mode in (gpu.RT_CAST_EXTEND_GLOBAL, gpu.RT_CAST_PACKET_GLOBAL):
        gp, gb, st = dev.cast_rays_ex(rays, mode)
        ties = compare_hits_with_oracle(orc, rays, op, ob, gp, gb, f"{name} mode {mode}")
        # random triangles never tie exactly; the boxes scene has shared edges (two triangles of a face, same t along the diagonal)
        assert ties <= (40 if name == "boxes" else 0), (name, mode, ties)
        # a subset of the reference's visits, and a real saving
        assert st["nodes_visited"] <= st_ref["nodes_visited"] and st["tri_tests"] <= st_ref["tri_tests"], (name, mode, st, st_ref)
    print(f"{name}: nodes visited global-best / reference = {st['nodes_visited']} / {st_ref['nodes_visited']} = {st['nodes_visited'] / st_ref['nodes_visited']:.4f}")


def test_guarded_rays_through_every_binary_kernel(pairs, gpu, oracle, sg):
    """Rays that leave the exact-reciprocal fast path (axis-parallel from box vertices; origin / direction components around 2^-40, 2^-37, 2^40)
    go through EVERY binary closest-hit kernel, shuffled among plain rays: all kernels take the guarded branch of the one inner-node step
    (trav_inner_apply, rt_dev_trav.h). The mix is checked per 64 consecutive rays: exactly a wave of the probe and of a packet, and the
    pool a refilling wave of wf_extend draws from. Parity modes: every field bit-equal to the oracle, and the packet kernel's counters are the per-lane
    kernel's ("by construction", rt_wf_extend.hip). Production modes: the hit contract; these rays are built to tie, so ties are not capped."""
    big = big_leaf_scene(sg)
    big_dev, big_orc = gpu.DeviceScene(big), oracle.OracleScene(big)
    try:
        info = big_dev.bvh_info(0)
        leaf_sizes = (info["nodes"][:, 9] - info["nodes"][:, 8])[info["nodes"][:, 6] == 0xFFFFFFFF]
        assert leaf_sizes.max() > 8, "the test needs a leaf beyond the cooperative limit (triangle-by-triangle walkers)"
        dev, orc, sc = pairs["boxes"]
        rdev, rorc, rsc = pairs["room_plain"]
        sets = [
            ("boxes", dev, orc, np.concatenate([degenerate_rays(sc), random_rays(sc, 2048 + 37, seed=511), _camera_rays(sc, 1024, seed=512)])),
            ("room_plain", rdev, rorc, fast_division_boundary_rays(rsc)),
            ("big_leaf", big_dev, big_orc, random_rays(big, 2000 + 37, seed=513)),
        ]
        for name, d, o, rays in sets:
            rays = rays[np.random.default_rng(514).permutation(len(rays))]
            g = is_guarded(rays)
            assert len(rays) % 64 != 0, f"{name}: the last wave must be partial"
            full = g[: len(g) // 64 * 64].reshape(-1, 64)
            assert (full.any(axis=1) & ~full.all(axis=1)).sum() >= len(full) // 2, f"{name}: guarded and plain rays must be mixed within 64 consecutive rays"
            op, ob = o.cast_rays(rays)
            stats = {}
            for mode in (gpu.RT_CAST_PROBE, gpu.RT_CAST_EXTEND, gpu.RT_CAST_PACKET):
                gp, gb, stats[mode] = d.cast_rays_ex(rays, mode)
                assert np.array_equal(gp, op), (name, mode, int((gp != op).sum()))
                assert np.array_equal(gb.view(np.uint32), ob.view(np.uint32)), (name, mode)
            for k in ("nodes_visited", "box_tests", "tri_tests"):
                assert stats[gpu.RT_CAST_EXTEND][k] == stats[gpu.RT_CAST_PACKET][k], (name, k, stats[gpu.RT_CAST_EXTEND][k], stats[gpu.RT_CAST_PACKET][k])
            for mode in (gpu.RT_CAST_EXTEND_GLOBAL, gpu.RT_CAST_PACKET_GLOBAL):
                gp, gb, _ = d.cast_rays_ex(rays, mode)
                compare_hits_with_oracle(o, rays, op, ob, gp, gb, f"guarded rays, {name} mode {mode}")
    finally:
        big_dev.close()
        big_orc.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_global_best_render_matches_oracle(pairs, gpu, name):
    """The whole pipeline with global-best traversal: same closest hits -> the oracle's framebuffer (1e-5 relative, the
    stated tolerance; a tie resolved differently would show up here as a different material / normal)."""
    dev, orc, _ = pairs[name]
    W, H, SPP = 48, 40, 6
    gfb, gst = dev.run_raytracer(W, H, SPP, seed=5, global_best=True, counters=True)
    ofb, ost = orc.run_raytracer(W, H, SPP, seed=5)
    rel = np.abs(gfb - ofb) / np.maximum(np.abs(ofb), 1e-6)
    assert rel.max() <= 1e-5, (name, float(rel.max()), int((rel > 1e-5).any(axis=2).sum()))
    bits = (gfb.view(np.uint32) != ofb.view(np.uint32)).any(axis=2)
    explain_pixels(orc, dev, W, H, SPP, 5, np.argwhere(bits), "exact", packet=False, global_best=True, what=f"{name}, global best")
    assert gst["casts"] == ost["casts"] and gst["shaded_hits"] == ost["shaded_hits"]  # same paths ...
    assert gst["nodes_visited"] <= ost["nodes_visited"]  # ... found with no more node visits


def test_global_best_on_the_bench_scene(gpu, oracle, sg):
    """S-sponza at full size (BASELINE config 3's scene): 60 000 rays and the 1000 x 1000 x 1 SPP framebuffer against the
    oracle; nodes / triangle tests per cast of both traversals are reported in the assertion messages' terms."""
    sc = sg.room_scene(262144, seed=0x5EED5EED, tex_size=64, n_tex_sets=16, n_materials=64, n_lights=16, light_strength=20.0,
                       alpha_fraction=0.02, offset=0.15, camera=sg.look_camera((-15.0, 4.0, 0.0), yaw_deg=-90.0, yfov=0.9))
    dev, orc = gpu.DeviceScene(sc), oracle.OracleScene(sc)
    try:
        rays = random_rays(sc, 60000, seed=4242)
        op, ob = orc.cast_rays(rays)
        _, _, st_ref = dev.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
        gp, gb, st = dev.cast_rays_ex(rays, gpu.RT_CAST_EXTEND_GLOBAL)
        assert compare_hits_with_oracle(orc, rays, op, ob, gp, gb, "S-sponza, global best", brute=1024) == 0
        assert st["nodes_visited"] <= st_ref["nodes_visited"], (st["nodes_visited"] / len(rays), st_ref["nodes_visited"] / len(rays))
        W = H = 1000
        gfb, gst = dev.run_raytracer(W, H, 1, seed=0x5EED5EED, global_best=True, counters=True)
        ofb, ost = orc.run_raytracer(W, H, 1, seed=0x5EED5EED)
        diff = (gfb.view(np.uint32) != ofb.view(np.uint32)).any(axis=2)
        assert not diff.any(), f"{int(diff.sum())} of 10^6 pixels differ from the oracle"
        assert gst["casts"] == ost["casts"]
        print(f"S-sponza nodes/cast {gst['nodes_visited'] / gst['casts']:.1f} (oracle {ost['nodes_visited'] / ost['casts']:.1f}), "
              f"triangle tests/cast {gst['tri_tests'] / gst['casts']:.1f} (oracle {ost['tri_tests'] / ost['casts']:.1f})")
    finally:
        dev.close()
        orc.close()


# ------------------------------------------------------------------------------------------------ RT_BUILD_WIDE
@pytest.fixture(scope="module")
def wide_pairs(gpu, oracle, scenes):
    out = {}
    for name, sc in scenes.items():
        out[name] = (gpu.DeviceScene(sc, wide=True), gpu.DeviceScene(sc, wide=True, device_bvh=True), oracle.OracleScene(sc), sc)
    yield out
    for a, b, o, _ in out.values():
        a.close()
        b.close()
        o.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_wide_tree_in_hbm_is_well_formed(wide_pairs, name):
    """What the kernels read (copied back from HBM), for the collapse of the reference-topology tree and of the device LBVH:
    every triangle in exactly one leaf slot, every quantised box contains its contents (tests/test_wide_build.py's walk)."""
    from test_wide_build import walk_and_check

    for dev in wide_pairs[name][:2]:
        sc = wide_pairs[name][3]
        d = dev.bvh_wide_dump()
        order = d["tris"][:, 9].copy()
        depth, hist = walk_and_check(d["nodes"], order, sc.positions)
        assert depth == d["depth"] and set(hist) <= {1, 2, 3}
        # the triangle records are the reference's operands (a, b - a, c - a) of exactly those triangles
        pos = sc.positions.reshape(-1, 9)[order]
        rec = d["tris"][:, :9].copy().view(np.float32)
        assert np.array_equal(rec[:, 0:3], pos[:, 0:3]) and np.array_equal(rec[:, 3:6], pos[:, 3:6] - pos[:, 0:3]) and np.array_equal(rec[:, 6:9], pos[:, 6:9] - pos[:, 0:3])


@pytest.mark.parametrize("name", FIXTURES)
def test_wide_hits_equal_the_oracle(wide_pairs, gpu, name):
    devh, devd, orc, sc = wide_pairs[name]
    rays = np.concatenate([random_rays(sc, 20000, seed=201), _camera_rays(sc, 8192, seed=202)])
    op, ob = orc.cast_rays(rays)
    for what, dev in (("host tree", devh), ("device LBVH", devd)):
        gp, gb, st = dev.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
        ties, closer = compare_superset_hits_with_oracle(orc, rays, op, ob, gp, gb, f"{name}, wide, {what}")
        # an index mismatch at bit-equal t is an exact tie: two triangles of a box face or wall along their shared diagonal, two
        # overlapping lights in one plane. The wide tree visits in another order than the reference's binary tree, so the
        # first-found rule (bvh.h:132) may keep the other one. Both kinds must stay rare on random rays.
        print(f"{name}, wide ({what}): {ties} exact ties resolved differently, {closer} hits closer than the reference's, of {len(rays)} rays")
        assert ties + closer <= len(rays) // 500 + (40 if name == "boxes" else 0), (name, what, ties, closer)
        assert st["nodes_visited"] > 0 and st["box_tests"] == 8 * st["nodes_visited"]
        gp2, gb2 = dev.cast_rays(rays)  # the plain probe entry point is routed through the same kernel on a wide scene
        assert np.array_equal(gp2, gp) and np.array_equal(gb2.view(np.uint32), gb.view(np.uint32))
        # the packet kernel (one walk per 64 consecutive rays, records through the scalar cache): coherent camera rays and, as a
        # stress, incoherent random ones; same superset contract, and the same hits as the per-lane kernel wherever no tie is involved
        pp, pb, pst = dev.cast_rays_ex(rays, gpu.RT_CAST_PACKET)
        pties, pcloser = compare_superset_hits_with_oracle(orc, rays, op, ob, pp, pb, f"{name}, wide packets, {what}")
        assert pties + pcloser <= len(rays) // 500 + (40 if name == "boxes" else 0), (name, what, pties, pcloser)
        assert np.array_equal(pb[:, 2].view(np.uint32), gb[:, 2].view(np.uint32)), "packet and per-lane wide traversal disagree on a closest-hit distance"
        assert pst["tri_tests"] > 0 and pst["nodes_visited"] >= st["nodes_visited"]  # a packet visits the union of its rays' nodes


def test_wide_degenerate_rays(wide_pairs, gpu):
    """Axis-parallel rays, rays starting ON box planes and vertices, zero direction components of either sign (the slab
    terms the wide kernel clamps instead of dividing by zero), on the axis-aligned boxes scene."""
    devh, _, orc, sc = wide_pairs["boxes"]
    v = sc.positions.reshape(-1, 3)
    rng = np.random.default_rng(9)
    o = v[rng.integers(0, len(v), size=6000)].astype(np.float32)
    d = np.zeros((6000, 3), dtype=np.float32)
    ax = rng.integers(0, 3, size=6000)
    d[np.arange(6000), ax] = rng.choice([-1.0, 1.0], size=6000)
    d[3000:, (ax[3000:] + 1) % 3] = rng.normal(size=3000).astype(np.float32)  # one exact zero left
    d[4500:] = np.where(d[4500:] == 0, np.float32(-0.0), d[4500:])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o[:1500] += rng.normal(scale=1e-3, size=(1500, 3)).astype(np.float32)
    rays = np.concatenate([o, d], axis=1).astype(np.float32)
    op, ob = orc.cast_rays(rays)
    gp, gb, _ = devh.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
    # rays IN the plane of a face are where exact and padded slabs may legitimately disagree (the reference's own outcome depends on
    # 0/0 = NaN compare order, bvh.h:141-145): such rays are counted, everything else must be the oracle's hit
    ot, gt = ob[:, 2].view(np.uint32), gb[:, 2].view(np.uint32)
    differ = (ot != gt) | ((op == 0xFFFFFFFF) != (gp == 0xFFFFFFFF))
    both = differ & (op != 0xFFFFFFFF) & (gp != 0xFFFFFFFF)
    only_gpu, only_orc = differ & (op == 0xFFFFFFFF), differ & (gp == 0xFFFFFFFF)
    print(f"degenerate rays: {int(differ.sum())} of {len(rays)} differ from the reference: {int(only_gpu.sum())} hit only by the wide traversal, "
          f"{int(only_orc.sum())} only by the reference, {int(both.sum())} both at another t ({int((gb[both, 2] < ob[both, 2]).sum())} closer)")
    # where they differ the wide traversal found a CLOSER (or the only) hit: it sees a superset of the reference's boxes
    assert (gb[both, 2] <= ob[both, 2]).all()
    assert not only_orc.any(), "the wide traversal missed a hit the reference finds"
    assert differ.mean() < 0.25, float(differ.mean())
    # and each of them exactly: every GPU-only and every closer hit is the returned triangle's own hit bit for bit, and on EVERY ray the wide
    # traversal's t is the brute-force minimum over all triangles (the hits the reference's NaN slab semantics lose are real)
    c = verify_hits(orc, rays, op, ob, gp, gb, "superset", what="degenerate rays")
    print(f"degenerate rays: {summary(c)}")
    assert c["verified"] >= int(only_gpu.sum() + both.sum()) and c["prod_ne_brute"] == 0


@pytest.mark.parametrize("name", FIXTURES)
def test_wide_render_matches_oracle(wide_pairs, gpu, name):
    devh, devd, orc, _ = wide_pairs[name]
    W, H, SPP = 48, 40, 6
    ofb, ost = orc.run_raytracer(W, H, SPP, seed=5)
    for what, dev in (("host tree", devh), ("device LBVH", devd)):
        gfb, gst = dev.run_raytracer(W, H, SPP, seed=5, counters=True)
        rel = np.abs(gfb - ofb) / np.maximum(np.abs(ofb), 1e-6)
        bad = (rel > 1e-5).any(axis=2)
        # every pixel that differs in ANY bit: one of its paths met a tie or a closer hit, verified exactly
        bits = (gfb.view(np.uint32) != ofb.view(np.uint32)).any(axis=2)
        recs = explain_pixels(orc, dev, W, H, SPP, 5, np.argwhere(bits), "superset", what=f"{name}, wide, {what}")
        print(f"{name}, wide ({what}): {len(recs)} pixels differ in some bit, all explained: "
              f"{sum(r['cause'] == 'exact tie' for r in recs)} by a tie, {len(recs) - sum(r['cause'] == 'exact tie' for r in recs)} by a closer hit")
        # 1e-5 relative wherever every cast of the pixel found the reference's own hit. A pixel may differ where a path met an
        # exact tie or a closer hit (see compare_superset_hits_with_oracle; light sampling aims rays AT the lights, two of which
        # overlap in one plane in some fixtures): such a path continues from another triangle. Bounded, and the image as a whole
        # is the same picture.
        print(f"{name}: {int(bad.sum())} of {W * H} pixels beyond 1e-5 relative; casts {gst['casts']} (oracle {ost['casts']})")
        assert bad.mean() <= 0.03, (name, int(bad.sum()))
        assert abs(float(gfb.mean()) - float(ofb.mean())) <= 0.02 * float(ofb.mean())
        assert abs(gst["casts"] - ost["casts"]) <= 0.002 * ost["casts"]
        assert gst["nodes_visited"] < ost["nodes_visited"]
    # shards, pass splitting and the rgb8 film do not care which tree is walked
    full, _ = devh.run_raytracer(W, H, SPP, seed=5)
    sh = np.zeros_like(full)
    for r in range(3):
        devh.run_raytracer(W, H, SPP, seed=5, shard_index=r, shard_count=3, shard_block=4 * W, out=sh)
    assert np.array_equal(sh.view(np.uint32), full.view(np.uint32))


def test_device_collapse_equals_host_collapse_of_the_same_tree(gpu, sg, monkeypatch):
    """RT_BUILD_WIDE on a device-built tree runs the collapse ON THE DEVICE (dynamic program inside the refit kernel, level-by-level
    emission). The same LBVH collapsed by wide_build.cpp on the host (RT_BUILD_WIDE_HOST_COLLAPSE) must give the same tree up to
    float-vs-double ties in the cost comparisons: same triangles, (almost) the same node count, depth and leaf-size histogram."""
    from test_wide_build import decode, walk_and_check

    sc = sg.room_scene(30000, seed=8, n_lights=4, n_materials=8, tex_size=0, offset=0.1)
    dev = gpu.DeviceScene(sc, wide=True, device_bvh=True)
    d1 = dev.bvh_wide_dump()
    t1 = dev.build_times()
    dev.close()
    dev = gpu.DeviceScene(sc, wide=True, device_bvh=True, build_flags=gpu.RT_BUILD_WIDE_HOST_COLLAPSE)
    d2 = dev.bvh_wide_dump()
    t2 = dev.build_times()
    dev.close()
    depth1, hist1 = walk_and_check(d1["nodes"], d1["tris"][:, 9].copy(), sc.positions)
    depth2, hist2 = walk_and_check(d2["nodes"], d2["tris"][:, 9].copy(), sc.positions)
    n1, n2 = len(d1["nodes"]), len(d2["nodes"])
    print(f"device collapse: {n1} nodes, depth {depth1}, leaf slots {hist1}, {t1['wide_ms']:.2f} ms; host collapse: {n2} nodes, depth {depth2}, leaf slots {hist2}, {t2['wide_ms']:.1f} ms")
    assert abs(n1 - n2) <= 0.01 * n2 and abs(depth1 - depth2) <= 1
    for k in (1, 2, 3):
        assert abs(hist1.get(k, 0) - hist2.get(k, 0)) <= 0.02 * sum(hist2.values())
    assert t1["wide_ms"] < t2["wide_ms"]


def test_packed_blob_decodes_to_the_builders_tree(gpu, sg):
    """The wide kernels read the PACKED tree (rt_wide_pack.hip: 64-byte nodes, origins as 3 x 20 bits on the scene grid, 4-bit exponents, slot
    states, nodes and triangle records in one blob). rt_bvh_wide_dump copies that blob back from HBM and decodes it; for a host-collapsed scene
    the result must be the host builder's own 80-byte tree (rt_bvh_wide_build_host on the same triangles), record for record — origin and
    exponents bit-equal (the builders snap to the grid, packing loses nothing), masks, all 48 plane bytes, children in slot order, every leaf
    slot's triangles — up to the order the records are numbered in. Also on a scene far from the origin (the grid's exact-float rule)."""
    from test_wide_build import assert_same_wide_tree

    for shift in (0.0, 3000.0):
        sc = sg.room_scene(20000, seed=9, n_lights=4, n_materials=8, tex_size=0, offset=0.1)
        sc.positions = (sc.positions.astype(np.float64) + shift).astype(np.float32)
        want = gpu.bvh_wide_build_host(sc.positions)
        dev = gpu.DeviceScene(sc, wide=True)
        got = dev.bvh_wide_dump()
        dev.close()
        assert len(want["order"]) == sc.n_triangles
        assert_same_wide_tree(got, want)  # tests/test_wide_build.py: shared with the deep trees of tests/test_gpu_deep_wide_walks.py


def test_wide_refuses_the_parity_modes(wide_pairs, gpu):
    devh = wide_pairs["room_plain"][0]
    with pytest.raises(gpu.RtError) as e:
        devh.run_raytracer(16, 16, 1, rng_mode=gpu.RT_RNG_REFERENCE)
    assert e.value.code == 8  # RT_ERR_UNSUPPORTED
    with pytest.raises(gpu.RtError):
        devh.run_raytracer(16, 16, 1, megakernel=True)
    with pytest.raises(gpu.RtError):
        devh.bvh_device_dump(0)
    assert devh.bvh_info(0)["nodes"].shape[0] > 0  # the binary tree it was collapsed from (host build) is still described


def test_wide_on_the_bench_scene(gpu, oracle, sg):
    """S-sponza at full size: 60 000 rays + the 1000 x 1000 x 1 SPP framebuffer against the oracle, for both binary sources."""
    sc = sg.room_scene(262144, seed=0x5EED5EED, tex_size=64, n_tex_sets=16, n_materials=64, n_lights=16, light_strength=20.0,
                       alpha_fraction=0.02, offset=0.15, camera=sg.look_camera((-15.0, 4.0, 0.0), yaw_deg=-90.0, yfov=0.9))
    orc = oracle.OracleScene(sc)
    rays = random_rays(sc, 60000, seed=4242)
    op, ob = orc.cast_rays(rays)
    W = H = 1000
    ofb, ost = orc.run_raytracer(W, H, 1, seed=0x5EED5EED)
    orc64 = orc
    # the parity-mode GPU image at the depth the bench quotes (64 SPP; itself pinned to the oracle by tests/test_gpu_parity.py): what the
    # production images are counted against below (the production numbers were proven at 1 SPP only)
    par = gpu.DeviceScene(sc)
    pfb64, _ = par.run_raytracer(W, H, 64, seed=0x5EED5EED)
    gbfb64, _ = par.run_raytracer(W, H, 64, seed=0x5EED5EED, global_best=True)
    n_gb = int((gbfb64.view(np.uint32) != pfb64.view(np.uint32)).any(axis=2).sum())
    print(f"S-sponza global-best pruning at 64 SPP: {n_gb} of 10^6 pixels differ from the parity image in any bit")
    assert n_gb == 0
    for what, kw in (("host tree", dict(wide=True)), ("device LBVH", dict(wide=True, device_bvh=True))):
        dev = gpu.DeviceScene(sc, **kw)
        try:
            wfb64, _ = dev.run_raytracer(W, H, 64, seed=0x5EED5EED)
            bits = (wfb64.view(np.uint32) != pfb64.view(np.uint32)).any(axis=2)
            rel = (np.abs(wfb64 - pfb64) / np.maximum(np.abs(pfb64), 1e-6)).max(axis=2)
            print(f"S-sponza wide ({what}) at the bench's 64 SPP (6.4e7 samples, ~2e8 casts): {int(bits.sum())} of 10^6 pixels differ from the parity image in any bit, "
                  f"{int((rel > 1e-5).sum())} beyond 1e-5 relative")
            assert int(bits.sum()) <= 2, (what, int(bits.sum()), np.argwhere(bits)[:8].tolist())  # measured: 0
            for rec in explain_pixels(orc64, dev, W, H, 64, 0x5EED5EED, np.argwhere(bits), "superset", brute=0, what=f"S-sponza wide ({what}), 64 SPP",
                                      parity=par):
                print(f"S-sponza wide ({what}):   {rec}")
            gp, gb, st = dev.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
            ties, closer = compare_superset_hits_with_oracle(orc, rays, op, ob, gp, gb, f"S-sponza, wide, {what}", brute=1024)
            assert ties + closer <= 6, (what, ties, closer)
            gfb, gst = dev.run_raytracer(W, H, 1, seed=0x5EED5EED, counters=True)
            diff = (gfb.view(np.uint32) != ofb.view(np.uint32)).any(axis=2)
            print(f"S-sponza wide ({what}): {ties} ties + {closer} closer hits of {len(rays)} rays; {int(diff.sum())} of 10^6 pixels differ from the oracle in any bit")
            assert diff.mean() <= 0.002, f"{what}: {int(diff.sum())} of 10^6 pixels differ from the oracle"
            explain_pixels(orc, dev, W, H, 1, 0x5EED5EED, np.argwhere(diff), "superset", packet=False, brute=0, what=f"S-sponza wide ({what}), 1 SPP")
            assert abs(gst["casts"] - ost["casts"]) <= 0.0005 * ost["casts"]
            print(f"S-sponza wide ({what}): wide nodes/cast {gst['nodes_visited'] / gst['casts']:.1f}, triangle tests/cast {gst['tri_tests'] / gst['casts']:.1f} "
                  f"(oracle, binary: {ost['nodes_visited'] / ost['casts']:.1f} / {ost['tri_tests'] / ost['casts']:.1f})")
        finally:
            dev.close()
    par.close()
    orc64.close()


# ------------------------------------------------------------------------------------------------ edge cases of the production build
def test_overlapping_coplanar_triangles_and_the_binary_production_trees(gpu, oracle, sg):
    """Found by tools/soak_parity.py (case 57): 40 random light triangles in ONE plane under the ceiling overlap each other, so a ray towards them
    has two candidate hits whose computed distances lie within an ulp of each other. The reference's pruning rule (bvh.h:216-223: skip the far child
    when its rounded slab-entry distance is >= the near hit) then decides by TREE SHAPE which of the two is found: the reference on its own tree
    returns one, the same rule on a device-built binary tree (or global-best culling) may return the other, one ulp FARTHER. Neither is wrong
    geometry. The contract this test pins for such scenes:
      * every production mode: hit / miss as the oracle; a differing t differs by <= 4 ulp, belongs to ANOTHER triangle, and is a true hit of that
        triangle (float64 recomputation written here: t within 1e-5 relative, barycentrics inside; and on every differing ray the oracle's own test
        of that triangle gives the returned (b, c, t) bit for bit);
      * the wide tree (conservative boxes, global best): never farther than the oracle, on any ray, and its t is the brute-force minimum;
      * the share of rays concerned is counted and bounded (they are rays into the overlap of two coplanar lights)."""
    sc = sg.room_scene(500, seed=1610353746, offset=1.5, n_lights=40, light_strength=5.0, n_materials=1, tex_size=0, n_tex_sets=1, alpha_fraction=0.0,
                       smooth_normals=True, camera=sg.look_camera((16.3, 14.9, -1.9), yaw_deg=42.0, yfov=1.1))
    rng = np.random.default_rng(57)
    n = 60_000
    o = np.stack([rng.uniform(-19, 19, n), rng.uniform(1, 14, n), rng.uniform(-9, 9, n)], axis=1)
    d = rng.normal(size=(n, 3)) * np.array([0.5, 0.0, 0.5]) + np.array([0.0, 1.0, 0.0])  # upwards, into the plane of the lights
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], axis=1).astype(np.float32)
    orc = oracle.OracleScene(sc)
    op, ob = orc.cast_rays(rays)
    assert (op != 0xFFFFFFFF).all()
    P = sc.positions.astype(np.float64)

    def true_hit(i, prim, t):  # float64 Cramer solution for ray i against triangle `prim`
        a, b, c = P[prim]
        oo, dd = rays[i, :3].astype(np.float64), rays[i, 3:].astype(np.float64)
        m = np.stack([b - a, c - a, -dd], axis=1)
        x = np.linalg.solve(m, oo - a)
        return x[0] >= -1e-6 and x[1] >= -1e-6 and x[0] + x[1] <= 1 + 1e-6 and abs(x[2] - t) <= 1e-5 * abs(t)

    def ulps(a, b):
        return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))

    report = []
    try:
        for what, build, mode, superset in (("reference tree, global best", {}, gpu.RT_CAST_EXTEND_GLOBAL, False), ("device PLOC tree", dict(device_bvh=True), gpu.RT_CAST_EXTEND, False),
                                            ("device PLOC tree, global best", dict(device_bvh=True), gpu.RT_CAST_EXTEND_GLOBAL, False),
                                            ("device radix tree", dict(device_bvh=True, device_builder=gpu.RT_BUILDER_LBVH), gpu.RT_CAST_EXTEND, False),
                                            ("wide tree, host collapse", dict(wide=True), gpu.RT_CAST_EXTEND, True), ("wide tree, device build", dict(wide=True, device_bvh=True), gpu.RT_CAST_EXTEND, True)):
            dev = gpu.DeviceScene(sc, **build)
            try:
                gp, gb, _ = dev.cast_rays_ex(rays, mode)
            finally:
                dev.close()
            assert np.array_equal(gp == 0xFFFFFFFF, op == 0xFFFFFFFF), what
            diff = np.flatnonzero(ob[:, 2].view(np.uint32) != gb[:, 2].view(np.uint32))
            farther = int((gb[diff, 2] > ob[diff, 2]).sum())
            assert ulps(ob[diff, 2], gb[diff, 2]).max(initial=0) <= 4, (what, int(ulps(ob[diff, 2], gb[diff, 2]).max()))
            assert (gp[diff] != op[diff]).all(), f"{what}: the SAME triangle with another t"
            for i in diff[:200]:
                assert true_hit(int(i), int(gp[i]), float(gb[i, 2])), (what, int(i), int(gp[i]))
            # exactly, on EVERY ray whose hit differs in any word: the returned triangle's own test gives that (b, c, t) bit for bit
            differ = np.flatnonzero((gp != op) | (gb.view(np.uint32) != ob.view(np.uint32)).any(axis=1))
            verify_reported_hits(orc, rays, gp, gb, differ, what=what)
            if superset:
                assert farther == 0, f"{what}: {farther} rays return a farther hit than the oracle"
                c = verify_hits(orc, rays, op, ob, gp, gb, "superset", what=what)  # and t is the brute-force minimum on every ray
                report.append(f"{what}: {summary(c)}")
            else:
                c = verify_hits(orc, rays, op, ob, gp, gb, "exact", what=what, coplanar_ulps=4)
                report.append(f"{what}: brute force: t_prod != t_brute on {c['prod_ne_brute']} rays, t_oracle > t_brute on {c['oracle_above_brute']}")
            assert len(diff) <= 2e-3 * n, (what, len(diff))
            ties = int(((gp != op) & (ob[:, 2].view(np.uint32) == gb[:, 2].view(np.uint32))).sum())
            report.append(f"{what}: {len(diff)} rays with another t ({farther} farther, <= 4 ulp), {ties} exact ties")
    finally:
        orc.close()
    print("\n[coplanar overlap, %d rays] " % n + "; ".join(report))


def _tiny_scene(sg, n_tris, seed):
    """n_tris triangles in front of a camera at the origin looking down -z; the last one is emissive."""
    rng = np.random.default_rng(seed)
    c = rng.uniform([-2.0, -1.5, -7.0], [2.0, 1.5, -4.0], size=(n_tris, 1, 3))
    pos = (c + rng.uniform(-2.0, 2.0, size=(n_tris, 3, 3)) * np.array([1.0, 1.0, 0.3])).astype(np.float32)
    mats = [sg.Material(color=(0.7, 0.6, 0.5, 1.0), roughness=0.6, metallic=0.2), sg.Material(color=(1, 1, 1, 1), emission=(1.0, 0.9, 0.8), emissive_strength=9.0, roughness=1.0, metallic=0.0)]
    ids = np.zeros(n_tris, dtype=np.uint32)
    ids[-1] = 1
    tang = np.tile(np.array([1, 0, 0], dtype=np.float32), (n_tris, 3, 1))
    return sg.Scene(positions=pos, normals=None, texcoords=rng.uniform(0, 1, size=(n_tris, 3, 2)).astype(np.float32), tangents=tang, material_ids=ids,
                    materials=mats, textures=[], camera=sg.look_camera((0.0, 0.0, 0.0), yaw_deg=0.0, yfov=0.9, aspect=32 / 24))


@pytest.mark.parametrize("n_tris", [0, 1, 2, 3, 4, 8, 9, 10, 17, 40])
def test_wide_on_tiny_scenes(gpu, oracle, sg, n_tris):
    """A root that is a single leaf slot, fewer children than slots, the switch between the host collapse (<= 8 triangles) and the
    device collapse (> 8), the empty scene: hits and renders against the oracle for both ways to build the wide tree."""
    sc = _tiny_scene(sg, n_tris, seed=100 + n_tris) if n_tris else sg.room_scene(0, seed=1, n_lights=0, open_room=True)
    orc = oracle.OracleScene(sc)
    rng = np.random.default_rng(n_tris)
    d = rng.normal(size=(4000, 3)).astype(np.float32) * np.array([1.0, 1.0, 0.4], dtype=np.float32) + np.array([0, 0, -1.0], dtype=np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([rng.normal(scale=0.5, size=(4000, 3)).astype(np.float32), d.astype(np.float32)], axis=1)
    op, ob = orc.cast_rays(rays)
    ofb, _ = orc.run_raytracer(32, 24, 4, seed=3)
    try:
        for kw in (dict(wide=True), dict(wide=True, device_bvh=True)):
            dev = gpu.DeviceScene(sc, **kw)
            try:
                for mode in (gpu.RT_CAST_EXTEND, gpu.RT_CAST_PACKET):
                    gp, gb, _ = dev.cast_rays_ex(rays, mode)
                    ties, closer = compare_superset_hits_with_oracle(orc, rays, op, ob, gp, gb, f"{n_tris} triangles {kw} mode {mode}")
                    assert ties + closer == 0, (n_tris, kw, mode, ties, closer)
                if n_tris:
                    dump = dev.bvh_wide_dump()
                    from test_wide_build import walk_and_check

                    walk_and_check(dump["nodes"], dump["tris"][:, 9].copy(), sc.positions)
                gfb, _ = dev.run_raytracer(32, 24, 4, seed=3)
                rel = np.abs(gfb - ofb) / np.maximum(np.abs(ofb), 1e-6)
                assert rel.max() <= 1e-5, (n_tris, kw, float(rel.max()))
                explain_pixels(orc, dev, 32, 24, 4, 3, np.argwhere((gfb.view(np.uint32) != ofb.view(np.uint32)).any(axis=2)), "superset", what=f"{n_tris} triangles {kw}")
            finally:
                dev.close()
    finally:
        orc.close()


def test_wide_build_refuses_scenes_outside_its_exponent_range(gpu, sg):
    """The packed wide node keeps cell exponents in 4 bits above a scene base and the kernels add them to a float's exponent field (rt_wide.hip, WRay):
    sound while the scene's largest cell exponent lies in [-60, 44]. Outside, rt_create refuses RT_BUILD_WIDE (RT_ERR_UNSUPPORTED) instead of building a
    tree whose arithmetic could leave the normal floats; the parity build of the same scene is created as before."""
    for scale_log2 in (60, -70):
        sc = sg.room_scene(200, seed=78, n_lights=2, n_materials=4, tex_size=0)
        k = np.float32(2.0) ** np.float32(scale_log2)
        sc.positions = (sc.positions * k).astype(np.float32)
        sc.camera.position = (np.asarray(sc.camera.position, dtype=np.float32) * k).astype(np.float32)
        assert np.isfinite(sc.positions).all() and (sc.positions != 0).any()
        for kw in (dict(wide=True), dict(wide=True, device_bvh=True)):
            with pytest.raises(gpu.RtError) as e:
                gpu.DeviceScene(sc, **kw)
            assert e.value.code == 8 and "exponent range" in str(e.value), (scale_log2, kw, str(e.value))
        gpu.DeviceScene(sc).close()


@pytest.mark.parametrize("scale_log2", [36, 20, -8])
def test_production_build_at_extreme_scales(gpu, oracle, sg, scale_log2):
    """The same room scaled by 2^36, 2^20 and 2^-8: every production build against the oracle — the superset contract on 12 000 rays, every
    wide box containing its contents in exact arithmetic, the render. 2^36 is the top of the range in which the reference's own arithmetic
    is sound for a scene of this size: from about 2^40 its triangle test's triple products overflow and it reports "hits" at t = inf
    (measured: 11 853 of 12 000 rays at 2^41). The parity kernels reproduce those (test_render_outside_fast_division_range); the production
    traversal culls against the best distance so far and reports a miss instead. Below 2^-8 the scene is smaller than the reference's
    minimum hit distance EPS and nothing is hit at all."""
    sc = sg.room_scene(400, seed=77, n_lights=3, n_materials=5, tex_size=0)
    k = np.float32(2.0) ** np.float32(scale_log2)
    sc.positions = (sc.positions * k).astype(np.float32)
    sc.camera.position = (np.asarray(sc.camera.position, dtype=np.float32) * k).astype(np.float32)
    assert np.isfinite(sc.positions).all()
    orc = oracle.OracleScene(sc)
    rays = random_rays(sc, 12000, seed=5)
    op, ob = orc.cast_rays(rays)
    assert (op != 0xFFFFFFFF).sum() > 8000 and np.isfinite(ob[op != 0xFFFFFFFF, 2]).all()
    ofb, _ = orc.run_raytracer(32, 24, 3, seed=3)
    try:
        for kw in (dict(wide=True), dict(wide=True, device_bvh=True), dict(device_bvh=True)):
            dev = gpu.DeviceScene(sc, **kw)
            try:
                gp, gb, _ = dev.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
                # the binary device tree: the superset bounds, and verified against the exact contract of a binary production tree
                ties, closer = compare_superset_hits_with_oracle(orc, rays, op, ob, gp, gb, f"scale 2^{scale_log2} {kw}", kind="superset" if kw.get("wide") else "exact")
                assert ties + closer <= 12, (scale_log2, kw, ties, closer)
                if kw.get("wide"):
                    dump = dev.bvh_wide_dump()
                    from test_wide_build import walk_and_check

                    walk_and_check(dump["nodes"], dump["tris"][:, 9].copy(), sc.positions)
                gfb, _ = dev.run_raytracer(32, 24, 3, seed=3)
                bits = (gfb.view(np.uint32) != ofb.view(np.uint32)).any(axis=2)
                differing = int(bits.sum())
                assert differing <= 8, (scale_log2, kw, differing)
                explain_pixels(orc, dev, 32, 24, 3, 3, np.argwhere(bits), "superset" if kw.get("wide") else "exact", packet=False, what=f"scale 2^{scale_log2} {kw}")
            finally:
                dev.close()
    finally:
        orc.close()


def test_wide_with_analytic_primitives(gpu, oracle, tmp_path):
    """Scene-txt scenes (BASELINE configs 1-2) through the production build: BOX / TRIANGLE primitives in the wide tree, ELLIPSOID /
    PLANE through wf_extend_prims after it; the oracle's image within 1e-5."""
    import os

    txt = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "txt", "cornell_mixed.txt")
    ls = gpu.parse_scene_txt(txt)
    orc = oracle.OracleScene(ls)
    ofb, ost = orc.run_raytracer(48, 40, 6, seed=4)
    try:
        for kw in (dict(wide=True), dict(wide=True, device_bvh=True)):
            dev = gpu.DeviceScene(ls, **kw)
            try:
                gfb, gst = dev.run_raytracer(48, 40, 6, seed=4, counters=True)
                rel = np.abs(gfb - ofb) / np.maximum(np.abs(ofb), 1e-6)
                assert (rel > 1e-5).any(axis=2).mean() <= 0.01, (kw, float(rel.max()))
                assert abs(gst["casts"] - ost["casts"]) <= 0.002 * ost["casts"]
                bits = (gfb.view(np.uint32) != ofb.view(np.uint32)).any(axis=2)
                recs = explain_pixels(orc, dev, 48, 40, 6, 4, np.argwhere(bits), "superset", what=f"cornell_mixed {kw}")
                print(f"cornell_mixed {kw}: {len(recs)} pixels differ from the oracle in some bit, all explained")
            finally:
                dev.close()
    finally:
        orc.close()


SCENE_TXT = ["cornell_mixed.txt", "practice3_5.txt", "scene-000.txt"]


@pytest.mark.parametrize("txt", SCENE_TXT)
def test_wide_hits_on_scene_txt(gpu, oracle, txt):
    """Scene-txt scenes through the wide tree, ray by ray: BOX / TRIANGLE primitives as triangles in the tree, ELLIPSOID / PLANE (indices >=
    n_triangles, reported (0, 0, t)) tested after it by wf_extend_prims. Both wide builds, per-lane and packet kernels, 20 000 random rays and
    8 192 camera rays: the superset contract with every differing hit verified bit for bit and t the brute-force minimum on every ray."""
    import os
    import types

    ls = gpu.parse_scene_txt(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "txt", txt))
    arrays = ls.arrays()
    orc = oracle.OracleScene(ls)
    try:
        pos = np.asarray(arrays["positions"], dtype=np.float32).reshape(-1, 3)
        n_tri = len(pos) // 3
        cam = types.SimpleNamespace(**arrays["camera"])
        pts = np.concatenate([pos, cam.position[None, :]])
        lo, hi = pts.min(axis=0) - 0.5, pts.max(axis=0) + 0.5
        rng = np.random.default_rng(303)
        o = rng.uniform(lo, hi, size=(20000, 3)).astype(np.float32)
        d = rng.normal(size=(20000, 3)).astype(np.float32)
        d[:1250] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, size=1250)] * rng.choice([-1.0, 1.0], size=(1250, 1)).astype(np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.concatenate([np.concatenate([o, d], axis=1).astype(np.float32), _camera_rays(types.SimpleNamespace(camera=cam), 8192, seed=304)])
        op, ob = orc.cast_rays(rays)
        n_prim_hits = int(((op != 0xFFFFFFFF) & (op >= n_tri)).sum())
        assert n_prim_hits > 0 and n_tri > 0
        for kw in (dict(wide=True), dict(wide=True, device_bvh=True)):
            dev = gpu.DeviceScene(ls, **kw)
            try:
                for mode in (gpu.RT_CAST_EXTEND, gpu.RT_CAST_PACKET):
                    gp, gb, _ = dev.cast_rays_ex(rays, mode)
                    c = verify_hits(orc, rays, op, ob, gp, gb, "superset", what=f"{txt} {kw} mode {mode}")
                    print(f"{txt} {kw} mode {mode} ({n_tri} triangles, {n_prim_hits} oracle hits on analytic primitives): {summary(c)}")
                    assert c["prod_ne_brute"] == 0
            finally:
                dev.close()
    finally:
        orc.close()
