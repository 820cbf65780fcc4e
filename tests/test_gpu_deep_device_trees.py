"""GPU tests of closest-hit walks that keep 36 to 45 frames pending, on trees the device's radix builder makes deep.

Every closest-hit kernel keeps its deferred siblings in a two-tier stack sized for RT_MAX_STACK = 64 frames (csrc/rt_dev_stack.h): registers
and LDS, then per-lane scratch (StackMemT) or the global workspace of the wavefront kernels' ring (RingStackT). The reference builder's SAH
tree cannot be made deep, so tests/test_gpu_deep_walks.py stops at 19 pending frames and positions 20..63 of the slow tier never ran in a test.
The Karras radix tree (rt_build_options.device_builder = RT_BUILDER_LBVH) is as deep as its keys are long: deep_walks.corner_ladder_scene gives
each of the 30 Morton bits a split whose two boxes both hold the scene's corner and ends the chain in 2^log2_soup equal codes there, which
the leaf-index bits split. A ray that starts inside all those boxes defers a sibling at every level.

Nothing about the depth is assumed: every test first walks the tree the DEVICE built (bvh_device_dump) with the reference's traversal rule
(deep_walks.dump_census) for its own rays and requires 90 % of them to keep at least 36 frames pending (main scene, 2^10 soup triangles) or
40 (second scene, 2^15). The oracle never sees these trees; it supplies the hits (its own SAH tree) and the brute-force minimum. Measured
on an MI355X (the tests print theirs; run with -s):

    scene    tree              depth   rays                     share at the required f    most pending
    main     radix             41      20 000 corner rays       100 % at f >= 36           40
    main     radix             41      48x32x2 primary rays     100 % at f >= 36           39
    second   radix             46      4 000 corner rays        100 % at f >= 40           45
    main     PLOC (no claim)   31      20 000 corner rays       -                          27
    main     8-wide tree collapsed from the radix tree: 144 nodes on 10 levels; its WALK is shallow, 5 node groups pending at most (a wide
             level absorbs about three binary levels and a chain's siblings are leaf slots): the ring of wf_extend_wide is never full
             there. Wide walks beyond the ring: tests/test_gpu_deep_wide_walks.py

Every comparison held on the first run: no hit differs from the oracle's in any bit, no tie, no pixel of the render differs.
"""
import numpy as np
import pytest

import deep_walks as dw
from hit_contract import explain_pixels, summary, verify_hits
from bvh_dump import check_invariants as _check_invariants, compare_hits_with_oracle as _compare_hits_with_oracle

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 48, 32, 2, 5
NINE_IN_TEN = 0.9
NO_TIES = 5e-5  # random triangles in general position do not tie (the bound tests/test_gpu_bvh_device.py uses for its random soups)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Corner:
    """One corner-ladder scene: in the oracle, on the device under the radix builder, its corner rays, the census of those rays on the device's
    own tree and the oracle's hits, all computed once."""

    def __init__(self, gpu, oracle, sg, spec, n_rays, need):
        self.name = f"corner ladder, 2^{spec['log2_soup']} soup"
        self.need = need
        self.log2_soup = spec["log2_soup"]
        self.sc = dw.corner_ladder_scene(sg, **spec)
        self.orc = oracle.OracleScene(self.sc)
        self.dev = gpu.DeviceScene(self.sc, device_bvh=True, device_builder=gpu.RT_BUILDER_LBVH)
        self.dump = self.dev.bvh_device_dump(0)
        self.rays = dw.corner_rays(dw.CORNER_CELL, n_rays, seed=7)
        self.counts = dw.dump_census(self.dump, self.rays)
        self.hits = self.orc.cast_rays(self.rays)

    def witnesses(self, what):
        return dw.require_witnesses(f"{self.name}, {what}", self.counts, self.need)

    def close(self):
        self.dev.close()
        self.orc.close()


@pytest.fixture(scope="module")
def main(gpu, oracle, sg):
    c = Corner(gpu, oracle, sg, dw.CORNER_MAIN, 20000, {36: NINE_IN_TEN})
    yield c
    c.close()


@pytest.fixture(scope="module")
def second(gpu, oracle, sg):
    c = Corner(gpu, oracle, sg, dw.CORNER_SECOND, 4000, {40: NINE_IN_TEN})
    yield c
    c.close()


@pytest.fixture(scope="module")
def corner(request, main):
    """`main`, or `second` for the tests parametrised with it (built only when one of them runs)."""
    return main if request.param == "main" else request.getfixturevalue("second")


def test_radix_tree_is_the_predicted_one(main):
    """k_keys, the 64-bit leaf keys, k_radix_tree and the bottom-up k_refit along a chain of 40 nodes: a proper BVH over all triangles with
    exact boxes, whose leaf order, child references and depth are those of the numpy restatement (deep_walks.radix_tree_dump)."""
    main.witnesses("corner rays")
    depth = _check_invariants(main.dump, main.sc.positions, max_leaf=1)
    model = dw.radix_tree_dump(main.sc.positions)
    assert np.array_equal(main.dump["tris"][:, 9], np.argsort(model["keys"], kind="stable")), "the leaf order is not the stable sort by Morton code"
    assert depth == dw.dump_depth(model) == dw.dump_depth(main.dump) == dw.CORNER_DEPTH[10]
    assert main.dump["root"] == model["root"]
    assert np.array_equal(main.dump["nodes"][:, :14], model["nodes"][:, :14]), "child boxes or references differ from the restated radix tree"
    assert np.array_equal(main.dump["tris"][:, :11], model["tris"][:, :11])
    print(f"[deep trees] {main.name}: {main.sc.n_triangles} triangles, radix tree {depth} deep")


@pytest.mark.parametrize("corner", ["main", "second"], indirect=True)
def test_probe_on_the_deep_radix_tree(corner):
    """cast_kernel (registers + StackMemT<12>: from the 14th pending frame on in per-lane scratch, here up to scratch position 31 of 52): t
    bit-equal to the oracle's on every ray, an index differs only as an exact tie, brute force on every ray."""
    corner.witnesses("probe")
    depth = dw.dump_depth(corner.dump)
    assert depth == dw.CORNER_DEPTH[corner.log2_soup]
    ties = _compare_hits_with_oracle(corner.orc, corner.dev, corner.rays, max_tie_share=NO_TIES, brute="all")
    assert (corner.hits[0] != 0xFFFFFFFF).mean() > 0.99  # the rays start inside the soup
    print(f"[deep trees] {corner.name}, probe: radix tree {depth} deep, tie share {ties:.1e}")


@pytest.mark.parametrize("corner", ["main", "second"], indirect=True)
def test_wavefront_kernels_on_the_deep_radix_tree(corner, gpu):
    """wf_extend and wf_extend_packet with their 6-deep ring evicting to the global workspace and refilling from it 30 times and more in a row
    (workspace positions up to 37, RingStackT::slot_of up to position 43): the probe's hits bit for bit (the same tree walked in the same
    order) and equal visit counts. The global-best variants under the "exact" contract, visiting no more nodes than the reference order."""
    corner.witnesses("wavefront casts")
    op, ob = corner.hits
    rays = corner.rays
    pp, pb = corner.dev.cast_rays(rays)
    stats = {}
    for mode in (gpu.RT_CAST_EXTEND, gpu.RT_CAST_PACKET):
        gp, gb, stats[mode] = corner.dev.cast_rays_ex(rays, mode)
        assert np.array_equal(gp, pp), (mode, int((gp != pp).sum()))
        assert np.array_equal(bits(gb), bits(pb)), (mode, int((bits(gb) != bits(pb)).any(axis=1).sum()))
    for k in ("nodes_visited", "box_tests", "tri_tests"):
        assert stats[gpu.RT_CAST_EXTEND][k] == stats[gpu.RT_CAST_PACKET][k] > 0, (k, stats[gpu.RT_CAST_EXTEND][k], stats[gpu.RT_CAST_PACKET][k])
    for mode in (gpu.RT_CAST_EXTEND_GLOBAL, gpu.RT_CAST_PACKET_GLOBAL):
        gp, gb, st = corner.dev.cast_rays_ex(rays, mode)
        c = verify_hits(corner.orc, rays, op, ob, gp, gb, "exact", brute="all", what=f"{corner.name}, mode {mode}")
        print(f"[deep trees] {corner.name}, mode {mode}: {summary(c)}")
        assert 0 < st["nodes_visited"] <= stats[gpu.RT_CAST_EXTEND]["nodes_visited"]


def test_renders_from_the_corner(main, gpu):
    """48x32 at 2 samples from the camera inside the soup: the primary rays (the device's own, rt_sensor_rays) keep the required frames
    pending on the device's tree; the wavefront image is the megakernel's bit for bit (ring + workspace against registers + LDS + scratch),
    and every pixel that differs from the oracle's image in any bit is explained by an exact tie on one of its paths."""
    main.witnesses("corner rays")
    sensor = gpu.Sensor.pinhole(main.sc.camera, seed=SEED)
    recs = main.dev.sensor_rays(sensor, W, H, SPP)
    primary = np.concatenate([recs["origin"], recs["dir"]], axis=1).astype(np.float32)
    assert primary.shape == (W * H * SPP, 6)
    dw.require_witnesses(f"{main.name}, primary rays of the render", dw.dump_census(main.dump, primary), main.need)
    ofb, _ = main.orc.run_raytracer(W, H, SPP, seed=SEED)
    wfb, _ = main.dev.run_raytracer(W, H, SPP, seed=SEED)
    mfb, _ = main.dev.run_raytracer(W, H, SPP, seed=SEED, megakernel=True)
    assert np.isfinite(wfb).all() and (ofb > 0).any(axis=2).mean() > 0.5  # not a black picture
    assert np.array_equal(bits(wfb), bits(mfb)), f"{int((bits(wfb) != bits(mfb)).any(axis=2).sum())} of {W * H} pixels differ between wavefront and megakernel"
    differ = (bits(wfb) != bits(ofb)).any(axis=2)
    recs = explain_pixels(main.orc, main.dev, W, H, SPP, SEED, np.argwhere(differ), "exact", brute="all", what=main.name)
    assert all(r["cause"] == "exact tie" for r in recs), recs
    print(f"[deep trees] {main.name}, render: {int(differ.sum())} of {W * H} pixels differ from the oracle in some bit, all explained by a tie")


def test_wide_tree_collapsed_from_the_deep_radix_tree(main, gpu):
    """The same radix tree as the input of the wide collapse (its dynamic program runs inside k_refit, along the 40-node chain), the device
    pack, and the level-by-level wide refit: wf_extend_wide and the wide packet kernel (one LDS stack level per tree level) under the
    "superset" contract, and a refit to the arrays the scene was created from changes no hit and no node. The depth asserted here is the
    BINARY tree's: the wide walk on the collapsed tree is shallow (its census is printed, without a claim) and stays inside the LDS ring of
    wf_extend_wide; tests/test_gpu_deep_wide_walks.py goes beyond it."""
    main.witnesses("corner rays (the binary tree the wide one is collapsed from)")
    op, ob = main.hits
    prod = gpu.DeviceScene(main.sc, wide=True, device_bvh=True, device_builder=gpu.RT_BUILDER_LBVH)
    try:
        before = prod.bvh_wide_dump()
        print(f"[deep trees] {main.name}: 8-wide tree of {len(before['nodes'])} nodes, {before['depth']} levels")
        dw.require_witnesses(f"{main.name}, node groups pending in the wide walk (no claim)", dw.wide_census(before, main.sc.positions, main.rays), {},
                             tag="deep trees", unit="groups", report=(dw.WIDE_RING_EVICT,))
        assert sorted(before["tris"][:, 9].tolist()) == list(range(main.sc.n_triangles))
        hits = {}
        for mode in (gpu.RT_CAST_EXTEND, gpu.RT_CAST_PACKET):
            gp, gb, st = prod.cast_rays_ex(main.rays, mode)
            c = verify_hits(main.orc, main.rays, op, ob, gp, gb, "superset", brute="all", what=f"{main.name}, wide, mode {mode}")
            print(f"[deep trees] {main.name}, wide, mode {mode}: {summary(c)}")
            assert st["nodes_visited"] > 0
            hits[mode] = (gp, gb)
        prod.update_geometry(main.sc, refit=True)
        after = prod.bvh_wide_dump()
        assert after["depth"] == before["depth"] and np.array_equal(after["nodes"], before["nodes"]) and np.array_equal(after["tris"], before["tris"])
        for mode, (gp, gb) in hits.items():
            rp, rb, _ = prod.cast_rays_ex(main.rays, mode)
            assert np.array_equal(rp, gp) and np.array_equal(bits(rb), bits(gb)), f"mode {mode}: a refit to the creation arrays changed {int((rp != gp).sum())} hits"
    finally:
        prod.close()


def test_ploc_on_the_corner_ladder(main, gpu):
    """The default builder on the same scene: a proper BVH and the probe contract. No depth is claimed for it (agglomerative clustering does
    not follow the Morton bits); the census of its tree is printed."""
    dev = gpu.DeviceScene(main.sc, device_bvh=True)
    try:
        dump = dev.bvh_device_dump(0)
        depth = _check_invariants(dump, main.sc.positions, max_leaf=4)
        dw.require_witnesses(f"{main.name}, PLOC tree {depth} deep, corner rays", dw.dump_census(dump, main.rays), {})
        _compare_hits_with_oracle(main.orc, dev, main.rays, max_tie_share=NO_TIES, brute="all")
    finally:
        dev.close()
