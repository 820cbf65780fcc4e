"""GPU tests of 8-wide closest-hit walks that keep 12 to 19 node groups pending: beyond the LDS ring of wf_extend_wide's stack.

wf_extend_wide (csrc/rt_wide.hip) keeps the newest pending group in registers, eight older ones in RingStackT<8, 2> in LDS and the rest in
the global overflow workspace; the 10th pending group is the first eviction (deep_walks.WIDE_RING_EVICT), and every refill from the
workspace happens on the way back from there. The wide packet kernel keeps one wave-uniform LDS entry per level. No other test gets
there: the wide tree collapsed from the 41-deep radix tree of tests/test_gpu_deep_device_trees.py has 10 levels and keeps 5 groups pending,
the needle soup of tests/test_gpu_deep_walks.py 6, and the host-collapsed tree of that corner scene stops at 9, the ring exactly full
(tests/test_wide_census.py pins it). The HOST-collapsed trees of the corner ladder with 2^13 and 2^15 soup triangles are 19 and 22 levels
deep, and rays from inside the soup keep 12 to 19 groups pending whatever their direction octant.

Nothing about that is assumed: every test first takes the census of its own rays on the tree the DEVICE holds (bvh_wide_dump, walked by
deep_walks.wide_census) and requires 90 % of them at 12 pending groups or more. 12 and not 10: the census tests the de-quantised boxes in
float64, the device tests conservative supersets of them with FMAs, so its walk may differ from the census by a box at a level or two;
two groups past the first eviction, it still evicts and refills. The oracle never sees these trees: it supplies the hits of its own SAH
tree and the brute-force minimum, under the wide tree's "superset" contract (tests/hit_contract.py). As printed on an MI355X (run with -s):

    scene       tree                 nodes / levels   rays                        share at >= 12    most pending
    2^13 soup   host collapse        835 / 19         4000 corner rays            100 %             14
    2^13 soup   host collapse        835 / 19         4000 octant rays            100 %             16
    2^15 soup   host collapse        3336 / 22        4000 corner rays            100 %             17
    2^15 soup   host collapse        3336 / 22        4000 octant rays            100 %             19
    2^13 soup   host collapse        835 / 19         48x32x2 primary rays        100 %             14
    2^13 soup   refitted, +-1e-3     835 / 19         4000 corner rays            100 %             14
    2^13 soup   device LBVH          1113 / 12        corner and octant rays      0 % (no claim)    6
    2^13 soup   device PLOC          850 / 12         corner and octant rays      0 % (no claim)    7 and 8

Every comparison held on the first run: no hit differs from the oracle's in any bit, no pixel of the render differs. That the device
really goes through the workspace was checked once with a build whose RingStackT::pop_masked cleared one pending bit of every group it
refilled from the workspace: the kernel, render, refit and interleaved-miss tests here then fail with "a production hit FARTHER than the
oracle's", while the device-built cases below and test_wide_tree_collapsed_from_the_deep_radix_tree (tests/test_gpu_deep_device_trees.py),
whose walks stay in the ring, still pass.
"""
import dataclasses

import numpy as np
import pytest

import deep_walks as dw
from hit_contract import explain_pixels, summary, verify_hits
from test_wide_build import assert_same_wide_tree, walk_and_check

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 48, 32, 2, 5
N_RAYS = 4000
NINE_IN_TEN = 0.9
CLAIM = {dw.WIDE_CLAIM: NINE_IN_TEN}
NONE = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def witnesses(what, counts, required=CLAIM):
    return dw.require_witnesses(what, counts, required, tag="deep wide", unit="groups", report=(dw.WIDE_RING_EVICT, dw.WIDE_CLAIM))


class Deep:
    """One corner-ladder scene: in the oracle, on the device under the host collapse, the dump of the device's tree, two ray sets, the census
    of each on that dump and the oracle's hits, all computed once."""

    def __init__(self, gpu, oracle, sg, spec):
        self.log2_soup = spec["log2_soup"]
        self.name = f"corner ladder, 2^{self.log2_soup} soup"
        self.sc = dw.corner_ladder_scene(sg, **spec)
        self.orc = oracle.OracleScene(self.sc)
        self.dev = gpu.DeviceScene(self.sc, wide=True)
        self.dump = self.dev.bvh_wide_dump()
        self.rays = {"corner rays": dw.corner_rays(dw.CORNER_CELL, N_RAYS, seed=7), "octant rays": dw.octant_rays(dw.CORNER_CELL, N_RAYS, seed=7)}
        self.counts = {k: dw.wide_census(self.dump, self.sc.positions, r) for k, r in self.rays.items()}
        self.hits = {k: self.orc.cast_rays(r) for k, r in self.rays.items()}

    def witnesses(self, kind, what):
        d = self.dump
        return witnesses(f"{self.name}, {len(d['nodes'])} nodes on {d['depth']} levels, {kind}, {what}", self.counts[kind])

    def close(self):
        self.dev.close()
        self.orc.close()


@pytest.fixture(scope="module")
def wide13(gpu, oracle, sg):
    c = Deep(gpu, oracle, sg, dw.CORNER_WIDE)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wide15(gpu, oracle, sg):
    c = Deep(gpu, oracle, sg, dw.CORNER_SECOND)
    yield c
    c.close()


@pytest.fixture(scope="module")
def deep(request, wide13):
    """`wide13`, or `wide15` for the tests parametrised with it (built only when one of them runs)."""
    return wide13 if request.param == 13 else request.getfixturevalue("wide15")


def cast_both_kernels(gpu, dev, orc, rays, op, ob, what):
    """The per-lane and the packet kernel on `rays` under the "superset" contract with brute force on every ray; the two kernels' hits are
    bit-equal to each other wherever no tie is involved: the same t on every ray, and the same (b, c) wherever they name the same triangle
    (a ray on which they name different triangles at one t is a tie, and verify_hits has checked both triangles' own tests bit for bit).
    Returns {mode: (prim, bct)}."""
    out = {}
    for mode, kernel in ((gpu.RT_CAST_EXTEND, "per-lane"), (gpu.RT_CAST_PACKET, "packet")):
        gp, gb, st = dev.cast_rays_ex(rays, mode)
        c = verify_hits(orc, rays, op, ob, gp, gb, "superset", brute="all", what=f"{what}, {kernel} kernel")
        print(f"[deep wide] {what}, {kernel} kernel: {summary(c)}; {st['nodes_visited'] / len(rays):.1f} nodes per ray")
        assert st["nodes_visited"] > 0
        out[mode] = (gp, gb)
    (ep, eb), (pp, pb) = out[gpu.RT_CAST_EXTEND], out[gpu.RT_CAST_PACKET]
    assert np.array_equal(bits(eb)[:, 2], bits(pb)[:, 2]) and np.array_equal(ep == NONE, pp == NONE), f"{what}: t differs between the two kernels"
    same = ep == pp
    assert np.array_equal(bits(eb)[same], bits(pb)[same]), f"{what}: (b, c) differ between the two kernels on a ray where both name one triangle"
    print(f"[deep wide] {what}: the two kernels name different triangles at one t on {int((~same).sum())} of {len(rays)} rays")
    return out


@pytest.mark.parametrize("kind", ["corner rays", "octant rays"])
@pytest.mark.parametrize("deep", [13, 15], indirect=True)
def test_wide_kernels_beyond_the_ring(deep, gpu, kind):
    """wf_extend_wide with its ring evicting to the workspace and refilling from it (positions up to 9 of the workspace on the larger scene,
    RingStackT<8, 2>::slot_of up to position 17) and the packet kernel, whose wave-uniform LDS stack holds a group while ANY lane has a
    slot of it pending and so is at least as deep as its deepest lane's, in one direction octant and in all eight (a packet of octant rays
    walks in the order of its first lane's octant)."""
    deep.witnesses(kind, "both wide kernels")
    op, ob = deep.hits[kind]
    assert (op != NONE).mean() > 0.99  # the rays start inside the soup
    cast_both_kernels(gpu, deep.dev, deep.orc, deep.rays[kind], op, ob, f"{deep.name}, {kind}")


def test_deep_dump_is_the_host_builders_tree(wide13, gpu):
    """The device pack (rt_wide_pack.hip) and its decoder on a 19-level tree: bvh_wide_dump is bvh_wide_build_host's tree record for record
    and order for order, the depth is the predicted one, and the dumped tree is a proper wide BVH over all triangles."""
    wide13.witnesses("corner rays", "dump against the host builder")
    want = gpu.bvh_wide_build_host(wide13.sc.positions)
    levels = assert_same_wide_tree(wide13.dump, want)
    assert levels == wide13.dump["depth"] == want["depth"] == dw.CORNER_WIDE_DEPTH[13]
    depth, _ = walk_and_check(wide13.dump["nodes"], wide13.dump["tris"][:, 9], wide13.sc.positions.reshape(-1, 9))
    assert depth == levels


# wf_extend_wide's persistent grid on an MI355X: 8 blocks of 4 waves on each of 256 CUs (rt_scene_impl.h wf_stack_stride). A wave takes its rays
# in chunks of 64 queue positions (RT_WIDE_CHUNK), one ticket per chunk.
GRID_WAVES = 256 * 8 * 4
COPIES_THAT_FORCE_REFILLS = (2 * GRID_WAVES * 64) // (2 * N_RAYS) + 1  # 132: twice as many chunks as the grid has waves


@pytest.mark.parametrize("copies", [1, COPIES_THAT_FORCE_REFILLS])
def test_queue_refill_among_deep_lanes(wide13, gpu, copies):
    """One cast of the corner rays interleaved one to one with rays that start outside the scene and point away: those end at the root, so every
    second lane of a wave is idle, or takes a fresh ray from the queue (wide_init, stk.reset()), while its neighbours are in the ring or
    beyond it. The deep half's hits are those of the cast without the misses, bit for bit; the other half misses.
    copies = 1: 4000 + 4000 rays, 125 chunks for a grid of 8192 waves. A wave needs no second ticket then, so whether a lane is refilled next to
    deep neighbours is left to the launch order. copies = 132: the 8000 rays 132 times over, 16 500 chunks, twice the waves of the grid: waves
    MUST take further chunks, and they take them when the 32 misses of a chunk have ended and its 32 deep rays have not. Every copy of a
    deep ray must get the hit of the plain cast, bit for bit."""
    wide13.witnesses("corner rays", f"interleaved with misses, {copies} times over")
    rays = wide13.rays["corner rays"]
    rng = np.random.default_rng(9)
    o = -rng.uniform(1.0, 2.0, size=(N_RAYS, 3))
    d = -rng.uniform(0.3, 1.0, size=(N_RAYS, 3))
    away = np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1).astype(np.float32)
    assert (wide13.orc.cast_rays(away)[0] == NONE).all()
    assert dw.wide_census(wide13.dump, wide13.sc.positions, away).max() == 0  # ... and nothing but the root's eight boxes is ever tested for them
    mixed = np.empty((copies, 2 * N_RAYS, 6), dtype=np.float32)
    mixed[:, 0::2], mixed[:, 1::2] = rays, away
    assert mixed.shape[0] * mixed.shape[1] // 64 > (1 if copies == 1 else 2 * GRID_WAVES)
    ap, ab, _ = wide13.dev.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
    assert (ap != NONE).mean() > 0.99
    mp, mb, st = wide13.dev.cast_rays_ex(mixed.reshape(-1, 6), gpu.RT_CAST_EXTEND)
    mp, mb = mp.reshape(copies, 2 * N_RAYS), bits(mb).reshape(copies, 2 * N_RAYS, 3)
    assert st["nodes_visited"] > 2 * copies * N_RAYS
    assert (mp[:, 1::2] == NONE).all() and not mb[:, 1::2].any(), f"{int((mp[:, 1::2] != NONE).sum())} rays that point away from the scene hit something"
    bad = (mp[:, 0::2] != ap[None]) | (mb[:, 0::2] != bits(ab)[None]).any(axis=2)
    assert not bad.any(), (f"{int(bad.sum())} of {bad.size} deep rays have another hit when every second lane of their wave holds a miss "
                           f"(first: copy {int(np.argwhere(bad)[0][0])}, ray {int(np.argwhere(bad)[0][1])})")
    if copies == 1:
        op, ob = wide13.hits["corner rays"]
        c = verify_hits(wide13.orc, rays, op, ob, mp[0, 0::2], mb[0, 0::2].view(np.float32), "superset", brute="all", what=f"{wide13.name}, corner rays interleaved with misses")
        print(f"[deep wide] {wide13.name}, corner rays interleaved with misses: {summary(c)}")
    print(f"[deep wide] {wide13.name}, {copies} x ({N_RAYS} corner rays + {N_RAYS} misses): {st['nodes_visited'] / (copies * N_RAYS) - 1:.1f} nodes per deep ray, every copy bit-equal")


def test_renders_from_inside_the_soup(wide13, gpu):
    """48x32 at 2 samples from the scene's camera, inside the soup: the primary rays (the device's own, rt_sensor_rays) keep the required
    groups pending on the device's tree, and every pixel that differs from the oracle's image in any bit is explained by a legal hit of the
    wide tree on one of its paths (a tie, or a closer hit the reference's pruning skips)."""
    sensor = gpu.Sensor.pinhole(wide13.sc.camera, seed=SEED)
    recs = wide13.dev.sensor_rays(sensor, W, H, SPP)
    primary = np.concatenate([recs["origin"], recs["dir"]], axis=1).astype(np.float32)
    assert primary.shape == (W * H * SPP, 6)
    witnesses(f"{wide13.name}, primary rays of the render", dw.wide_census(wide13.dump, wide13.sc.positions, primary))
    ofb, _ = wide13.orc.run_raytracer(W, H, SPP, seed=SEED)
    gfb, _ = wide13.dev.run_raytracer(W, H, SPP, seed=SEED)
    assert np.isfinite(gfb).all() and (ofb > 0).any(axis=2).mean() > 0.4 and (gfb > 0).any(axis=2).mean() > 0.4  # not a black picture
    differ = (bits(gfb) != bits(ofb)).any(axis=2)
    recs = explain_pixels(wide13.orc, wide13.dev, W, H, SPP, SEED, np.argwhere(differ), "superset", brute="all", what=f"{wide13.name}, wide render")
    assert len(recs) == int(differ.sum())
    ties = sum(r["cause"] == "exact tie" for r in recs)
    print(f"[deep wide] {wide13.name}, render: {int(differ.sum())} of {W * H} pixels differ from the oracle in some bit, all explained: {ties} by a tie, "
          f"{len(recs) - ties} by a closer hit")


def moved_positions(positions, seed):
    """Every vertex moved by a uniform +-1e-3 cell per coordinate; coordinates stay 0 or within the traversal's exact fast-division range
    [2^-37, 2^40] (what falls below 2^-37, the corner pin's vertices, becomes 0)."""
    rng = np.random.default_rng(seed)
    m = positions.astype(np.float64) + rng.uniform(-1e-3, 1e-3, size=positions.shape) * dw.CORNER_CELL
    m = np.minimum(np.where(m < 2.0 ** -37, 0.0, m), 2.0 ** 40).astype(np.float32)
    nz = m[m != 0]
    assert (m >= 0).all() and nz.min() >= 2.0 ** -37 and nz.max() <= 2.0 ** 40
    return m


def test_refit_of_the_deep_tree(wide13, gpu, oracle):
    """The level-by-level wide refit (rt_wide_refit.hip) on 19 levels: a refit to the creation arrays changes no node and no hit; a refit to
    moved vertices gives the CPU model's records (bvh_wide_refit_host of the previous dump), a proper wide BVH of the moved triangles on which
    the rays still go beyond the ring, and hits under the wide tree's contract against an oracle of the moved scene."""
    sc, rays = wide13.sc, wide13.rays["corner rays"]
    dev = gpu.DeviceScene(sc, wide=True)
    try:
        before = dev.bvh_wide_dump()
        assert np.array_equal(before["nodes"], wide13.dump["nodes"]) and np.array_equal(before["tris"], wide13.dump["tris"])
        wide13.witnesses("corner rays", "before the refit")
        hits = {mode: dev.cast_rays_ex(rays, mode)[:2] for mode in (gpu.RT_CAST_EXTEND, gpu.RT_CAST_PACKET)}
        dev.update_geometry(sc, refit=True)
        same = dev.bvh_wide_dump()
        assert same["depth"] == before["depth"] and np.array_equal(same["nodes"], before["nodes"]) and np.array_equal(same["tris"], before["tris"])
        for mode, (gp, gb) in hits.items():
            rp, rb, _ = dev.cast_rays_ex(rays, mode)
            assert np.array_equal(rp, gp) and np.array_equal(bits(rb), bits(gb)), f"mode {mode}: a refit to the creation arrays changed {int((rp != gp).sum())} hits"
        moved = dataclasses.replace(sc, positions=moved_positions(sc.positions, seed=5))
        dev.update_geometry(moved, refit=True)
        after = dev.bvh_wide_dump()
        order = before["tris"][:, 9]
        model = gpu.bvh_wide_refit_host(before["nodes"], order, moved.positions)
        assert (model != before["nodes"]).any(axis=1).mean() > 0.9  # the move is not lost in the quantisation: nearly every node changes
        assert np.array_equal(after["nodes"], model), f"{int((after['nodes'] != model).any(axis=1).sum())} of {len(model)} nodes differ from bvh_wide_refit_host"
        assert after["depth"] == before["depth"] and np.array_equal(after["tris"][:, 9:], before["tris"][:, 9:])
        depth, _ = walk_and_check(after["nodes"], order, moved.positions.reshape(-1, 9))
        assert depth == dw.CORNER_WIDE_DEPTH[13]
        witnesses(f"{wide13.name}, refitted to vertices moved by +-1e-3 cell, corner rays", dw.wide_census(after, moved.positions, rays))
        orc = oracle.OracleScene(moved)
        try:
            op, ob = orc.cast_rays(rays)
            cast_both_kernels(gpu, dev, orc, rays, op, ob, f"{wide13.name}, refitted")
        finally:
            orc.close()
    finally:
        dev.close()


# Trees the device builds and collapses itself: the hit contract holds whatever they look like, and no depth is claimed. A radix tree's wide
# collapse stays in the ring (tests/deep_walks.py, "the census of the 8-wide walk": CORNER_MAIN's keeps 5 groups pending, this scene's 6 on the
# CPU restatement); PLOC's is whatever the clustering makes it. The census of each is printed.
DEVICE_BUILDERS = {"lbvh": "RT_BUILDER_LBVH", "ploc": None}


@pytest.mark.parametrize("builder", sorted(DEVICE_BUILDERS))
def test_device_built_wide_trees_of_the_same_scene(wide13, gpu, builder):
    opts = {"device_builder": getattr(gpu, DEVICE_BUILDERS[builder])} if DEVICE_BUILDERS[builder] else {}
    dev = gpu.DeviceScene(wide13.sc, wide=True, device_bvh=True, **opts)
    try:
        dump = dev.bvh_wide_dump()
        depth, _ = walk_and_check(dump["nodes"], dump["tris"][:, 9], wide13.sc.positions.reshape(-1, 9))
        assert depth == dump["depth"]
        for kind, rays in wide13.rays.items():
            counts = dw.wide_census(dump, wide13.sc.positions, rays)
            witnesses(f"{wide13.name}, {builder} tree collapsed on the device, {len(dump['nodes'])} nodes on {depth} levels, {kind} (no claim)", counts, {})
            op, ob = wide13.hits[kind]
            cast_both_kernels(gpu, dev, wide13.orc, rays, op, ob, f"{wide13.name}, {builder} tree collapsed on the device, {kind}")
    finally:
        dev.close()
