"""The device builders of csrc/rt_bvh_device.hip (keys, leaves, radix tree), csrc/rt_bvh_ploc.hip (k_ploc_*) and csrc/rt_bvh_collapse.hip (the
wide tree) held from the inside. tests/test_gpu_bvh_device.py accepts any proper BVH that finds the oracle's
hits; here the tree read back from HBM (rt_bvh_device_dump) is compared, exactly, with what the builder is DEFINED to build (tests/lbvh_replay.py):

  a. the records are in stable Morton order of the float32 keys (k_bounds, k_keys, the sort, k_leaves), also far from the origin and on a planar
     scene, where k_keys' zero-extent arm is taken;
  b. the radix builder's tree is the radix tree of the 64-bit leaf keys, node index for node index, leaf references included (k_radix_tree,
     leaf_ref), also where (almost) all Morton keys are equal and the tree lives on the leaf-index half of its keys;
  c. PLOC builds the largest-gap tree of a ruler scene for every search radius (the area criterion, the tie rule, k_ploc_merge,
     k_ploc_compact), which also proves that PLOC ran; and on a scattered soup, where the order of the merges matters, the tree of the replayed
     rounds (k_ploc_nn's LDS halo across block boundaries);
  d. rt_build_options.lbvh_leaf_tris and ploc_radius: full, partial and single-triangle last leaves, the clamps, the wide tree ignoring them;
  e. device builds whose coordinates leave the fast-division range (fast_bad -> DeviceBvh::fast_ok);
  f. one build big enough that every grid-stride loop takes a second trip."""
import functools
import time

import numpy as np
import pytest

import lbvh_replay as lr
from bvh_dump import LEAF, MASK, check_invariants, compare_hits_with_oracle
from conftest import random_rays
from hit_contract import explain_pixels

pytestmark = pytest.mark.gpu

NO_MORE_TIES_THAN = 5e-5


def _soup_scene(sg, pos, camera=None):
    n = len(pos)
    tan = np.tile(np.array([1, 0, 0], dtype=np.float32), (n, 3, 1))
    return sg.Scene(positions=np.ascontiguousarray(pos, dtype=np.float32), normals=None, texcoords=np.zeros((n, 3, 2), np.float32), tangents=tan,
                    material_ids=np.zeros(n, np.uint32), materials=[sg.Material(color=(0.7, 0.7, 0.7, 1.0), roughness=1.0, metallic=0.0)], textures=[],
                    camera=camera or sg.look_camera((0.0, 0.0, 6.0), yaw_deg=0.0, yfov=0.9))


def _random_soup(sg, n, seed):
    """As the tiny_* cases of tests/test_gpu_bvh_device.py."""
    return _soup_scene(sg, np.random.default_rng(seed).uniform(-2, 2, size=(n, 3, 3)))


ONE_CELL_LO, ONE_CELL_SIDE, ONE_CELL_EXTENT = 32.0 + 1.0 / 64, 1.0 / 64, 64.0


@functools.lru_cache(maxsize=None)
def _scene(sg, name):
    if name == "room_5000":
        return sg.room_scene(5000, seed=3, n_lights=6, n_materials=8, tex_size=8, n_tex_sets=2, offset=0.15)
    if name == "room_5000_shifted":
        sc = sg.room_scene(5000, seed=3, n_lights=6, n_materials=8, tex_size=8, n_tex_sets=2, offset=0.15)
        sc.positions = (sc.positions.astype(np.float64) + 3000.0).astype(np.float32)
        return sc
    if name == "planar":  # 45 x 45 small triangles on a jittered grid in the plane z = 0.5, each inside its own unit cell
        rng = np.random.default_rng(7)
        g = np.stack(np.meshgrid(np.arange(45.0), np.arange(45.0), indexing="ij"), axis=-1).reshape(-1, 1, 2)
        xy = g + 0.5 + rng.uniform(-0.2, 0.2, size=(len(g), 1, 2)) + rng.uniform(-0.15, 0.15, size=(len(g), 3, 2))
        pos = np.concatenate([xy, np.full((len(g), 3, 1), 0.5)], axis=2).astype(np.float32)
        lo, hi = lr.scene_bounds(pos)
        assert lo[2] == hi[2] and lr.morton_cells(pos)[1][2] == 0  # the z bounds coincide: inv[2] = 0 is taken
        assert (np.floor(pos[..., :2]) == g).all()  # no triangle leaves its cell: none touches another
        return _soup_scene(sg, pos, sg.look_camera((22.0, 22.0, 30.0), yaw_deg=0.0, yfov=0.9))
    if name == "one_cell":  # 300 triangles inside a cube of 1 / 4096 of the extent, two anchors spanning the bounds
        rng = np.random.default_rng(9)
        tri = rng.uniform(ONE_CELL_LO, ONE_CELL_LO + ONE_CELL_SIDE, size=(300, 3, 3))
        a0 = np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0]], dtype=np.float64)
        pos = np.concatenate([a0[None], tri, (ONE_CELL_EXTENT - a0)[None]]).astype(np.float32)
        lo, hi = lr.scene_bounds(pos)
        assert (lo == 0).all() and (hi == ONE_CELL_EXTENT).all() and ONE_CELL_SIDE * 4096 == ONE_CELL_EXTENT
        assert len(np.unique(lr.morton_keys(pos))) <= 3  # the tree over the 300 lives on the leaf-index half of the keys
        mid = ONE_CELL_LO + ONE_CELL_SIDE / 2
        return _soup_scene(sg, pos, sg.look_camera((mid, mid, mid + 4 * ONE_CELL_SIDE), yaw_deg=0.0, yfov=0.9))
    if name.startswith("soup_"):
        n = int(name.split("_")[1])
        return _random_soup(sg, n, seed=n)
    raise KeyError(name)


def _builder_opts(gpu, builder):
    return {"device_builder": gpu.RT_BUILDER_LBVH} if builder == "lbvh" else {}


def _dump_of(gpu, sc, **opts):
    dev = gpu.DeviceScene(sc, device_bvh=True, **opts)
    try:
        return dev.bvh_device_dump(0)
    finally:
        dev.close()


def _leaf_refs(dump):
    if dump["root"] & LEAF:
        return np.array([dump["root"]], dtype=np.uint32)
    kids = dump["nodes"][:, 12:14].reshape(-1)
    kids = kids[(kids & LEAF) != 0]
    return kids[np.argsort(kids & MASK)]  # by first record


def _render_contract(orc, dev, W, H, SPP, what):
    """The wavefront and the megakernel image of the device-built tree are bit-equal, and every pixel that differs from the oracle's in any bit
    has a path whose first differing hit is an exact tie."""
    a, _ = orc.run_raytracer(W, H, SPP, seed=5)
    b, _ = dev.run_raytracer(W, H, SPP, seed=5)
    m, _ = dev.run_raytracer(W, H, SPP, seed=5, megakernel=True)
    assert np.isfinite(b).all() and np.array_equal(b.view(np.uint32), m.view(np.uint32))
    bits = (a.view(np.uint32) != b.view(np.uint32)).any(axis=2)
    recs = explain_pixels(orc, dev, W, H, SPP, 5, np.argwhere(bits), "exact", packet=False, brute="all", what=what)
    assert all(r["cause"] == "exact tie" for r in recs), recs
    return int(bits.sum())


# ---- a. leaf order ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf_tris", [1, 3])
@pytest.mark.parametrize("builder", ["ploc", "lbvh"])
@pytest.mark.parametrize("name", ["room_5000", "room_5000_shifted", "planar"])
def test_leaf_order_is_the_stable_morton_order(gpu, sg, name, builder, leaf_tris):
    sc = _scene(sg, name)
    dump = _dump_of(gpu, sc, lbvh_leaf_tris=leaf_tris, **_builder_opts(gpu, builder))
    want = lr.leaf_order(lr.morton_keys(sc.positions))
    assert np.array_equal(dump["tris"][:, 9], want), f"{int((dump['tris'][:, 9] != want).sum())} of {len(want)} records are not where the stable Morton order puts them"


# ---- b. the radix tree -----------------------------------------------------------------------------------------------------------------------
def _assert_radix_tree(dump, positions, leaf_tris):
    """The dump of an RT_BUILDER_LBVH build equals the radix tree of the replayed keys. Returns (walk, keys64)."""
    n, L = len(positions), int(leaf_tris)
    keys = lr.morton_keys(positions)
    order = lr.leaf_order(keys)
    assert np.array_equal(dump["tris"][:, 9], order)
    k64 = lr.leaf_keys64(keys[order], L)
    n_leaves = (n + L - 1) // L
    assert len(k64) == n_leaves and len(dump["nodes"]) == n_leaves - 1
    walk = lr.walk_binary(dump)
    if n_leaves == 1:
        assert dump["root"] == LEAF | n << 27
        return walk, k64
    first, last, split = lr.radix_tree_arrays(k64)
    left, right = lr.radix_children(first, last, split, n, L)
    assert dump["root"] == 0
    for side, got, want in (("left", dump["nodes"][:, 12], left), ("right", dump["nodes"][:, 13], right)):
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"{len(bad)} inner nodes have another {side} child than the radix tree, first: node {bad[0]}: {got[bad[0]]:#x}, expected {want[bad[0]]:#x}"
    # and the same through the walk: node i covers the records of leaves [first, last], split after leaf `split`
    assert walk["contiguous"]
    assert np.array_equal(walk["lfirst"], first * L) and np.array_equal(walk["llast"], np.minimum((split + 1) * L, n) - 1)
    assert np.array_equal(walk["rfirst"], (split + 1) * L) and np.array_equal(walk["rlast"], np.minimum((last + 1) * L, n) - 1)
    return walk, k64


@pytest.mark.parametrize("leaf_tris", [1, 2, 8])
@pytest.mark.parametrize("name", ["room_5000", "planar", "soup_2", "soup_3", "soup_9", "one_cell"])
def test_radix_tree_is_its_definition(gpu, oracle, sg, name, leaf_tris):
    sc = _scene(sg, name)
    dev = gpu.DeviceScene(sc, device_bvh=True, device_builder=gpu.RT_BUILDER_LBVH, lbvh_leaf_tris=leaf_tris)
    try:
        dump = dev.bvh_device_dump(0)
        walk, _ = _assert_radix_tree(dump, sc.positions, leaf_tris)
        if name != "one_cell":
            return
        depth = check_invariants(dump, sc.positions, max_leaf=leaf_tris)
        # half the rays as everywhere, half aimed at the cube from around it (the scene is empty but for the cube)
        rng = np.random.default_rng(4)
        mid = ONE_CELL_LO + ONE_CELL_SIDE / 2
        o = rng.uniform(mid - 2 * ONE_CELL_SIDE, mid + 2 * ONE_CELL_SIDE, size=(10_000, 3))
        d = rng.uniform(ONE_CELL_LO, ONE_CELL_LO + ONE_CELL_SIDE, size=(10_000, 3)) - o
        aimed = np.concatenate([o, d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1).astype(np.float32)
        rays = np.concatenate([random_rays(sc, 10_000, seed=12), aimed])
        orc = oracle.OracleScene(sc)
        try:
            assert (orc.cast_rays(aimed)[0] != 0xFFFFFFFF).mean() > 0.5  # the aimed rays do meet the cube's triangles
            ties = compare_hits_with_oracle(orc, dev, rays, max_tie_share=NO_MORE_TIES_THAN)
        finally:
            orc.close()
        print(f"\n[one cell, {leaf_tris} per leaf] depth {depth}, height {walk['height']}, tie share {ties:.2e}")
    finally:
        dev.close()


# ---- c. PLOC ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 8, 32])
@pytest.mark.parametrize("n,offset", [(600, 0), (600, 1), (257, 255), (513, 3)])
def test_ploc_builds_the_largest_gap_tree(gpu, oracle, sg, n, offset, radius):
    """The first rounds merge mutual pairs on both sides of k_ploc_nn's 256-cluster block boundary (positions 255 | 256, 511 | 512 with these
    sizes and offsets); radius 32 reads the whole halo. tests/test_lbvh_replay.py shows that the rounds as specified build this tree."""
    sc, x = lr.ruler_scene(sg, n, offset)
    want = lr.largest_gap_tree(x)
    dev = gpu.DeviceScene(sc, device_bvh=True, **({} if radius == 8 else {"ploc_radius": radius}))
    try:
        dump = dev.bvh_device_dump(0)
        assert np.array_equal(dump["tris"][:, 9], np.arange(n))
        assert lr.nested(dump) == want  # left / right included; the radix tree of these keys is another tree, so PLOC ran
        if (n, offset) == (600, 1):
            check_invariants(dump, sc.positions, max_leaf=1)
            orc = oracle.OracleScene(sc)
            try:
                compare_hits_with_oracle(orc, dev, random_rays(sc, 20_000, seed=12), max_tie_share=NO_MORE_TIES_THAN)
            finally:
                orc.close()
    finally:
        dev.close()


def _drifting_soup(sg, n):
    """n small triangles scattered in a cube: unlike on the ruler, WHEN a pair merges decides what its neighbours do next."""
    rng = np.random.default_rng(n)
    return _soup_scene(sg, rng.uniform(0, 10, size=(n, 1, 3)) + rng.uniform(-0.3, 0.3, size=(n, 3, 3)), sg.look_camera((5.0, 5.0, 25.0), yaw_deg=0.0, yfov=0.9))


@pytest.mark.parametrize("radius", [1, 8, 32])
@pytest.mark.parametrize("n", [257, 600])
def test_ploc_rounds_are_the_replayed_rounds(gpu, sg, n, radius):
    """The ruler tree does not depend on the ORDER of the merges: a cluster at a block boundary that k_ploc_nn shows the wrong neighbours only
    merges a round late there, and the same tree comes out (measured: a halo filled with the block's first box passes the test above). On a
    scattered soup a late merge changes what the neighbours choose, so here the tree must be the one lbvh_replay.ploc_replay builds round by
    round from the same boxes in the same order. The replay is exact: the build compiles without FMA contraction, so every area is the float32
    value the replay computes, operation for operation."""
    sc = _drifting_soup(sg, n)
    order = lr.leaf_order(lr.morton_keys(sc.positions))
    want, rounds, forced = lr.ploc_replay(lr.triangle_boxes(sc.positions[order]), radius)
    dump = _dump_of(gpu, sc, ploc_radius=radius)
    assert np.array_equal(dump["tris"][:, 9], order)
    assert lr.nested(dump) == want, f"radius {radius}: not the tree of the replay's {rounds} rounds ({forced} forced)"
    check_invariants(dump, sc.positions, max_leaf=1)


def test_ruler_radix_tree_is_another_tree(gpu, sg):
    """What the equality above proves: on the same scene the radix builder gives its own tree, not the largest-gap tree."""
    sc, x = lr.ruler_scene(sg, 600, 1)
    dump = _dump_of(gpu, sc, device_builder=gpu.RT_BUILDER_LBVH)
    _assert_radix_tree(dump, sc.positions, 1)
    assert lr.nested(dump) != lr.largest_gap_tree(x)


# ---- d. options ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["ploc", "lbvh"])
@pytest.mark.parametrize("leaf_tris,delta", [(L, d) for L in (2, 3, 8) for d in (-1, 0, 1)])
def test_leaf_size_matrix(gpu, oracle, sg, leaf_tris, delta, builder):
    """256, 256 and 257 leaves whose last one holds L - 1, L and 1 triangles."""
    L = leaf_tris
    n = 256 * L + delta
    sc = _scene(sg, f"soup_{n}")
    n_leaves = (n + L - 1) // L
    orc = oracle.OracleScene(sc)
    dev = gpu.DeviceScene(sc, device_bvh=True, lbvh_leaf_tris=L, **_builder_opts(gpu, builder))
    try:
        dump = dev.bvh_device_dump(0)
        depth = check_invariants(dump, sc.positions, max_leaf=L)
        refs = _leaf_refs(dump)
        assert np.array_equal(refs & MASK, np.arange(n_leaves) * L)
        assert ((refs[:-1] >> 27) & 15 == L).all() and (refs[-1] >> 27) & 15 == n - L * (n_leaves - 1) == (L - 1, L, 1)[delta + 1]
        if builder == "lbvh":
            _assert_radix_tree(dump, sc.positions, L)
        ties = compare_hits_with_oracle(orc, dev, random_rays(sc, 20_000, seed=12), max_tie_share=NO_MORE_TIES_THAN)
        differing = _render_contract(orc, dev, 48, 32, 4, f"soup of {n}, {L} per leaf, {builder}")
        print(f"\n[{n} triangles, {L} per leaf, {builder}] depth {depth}, tie share {ties:.2e}, {differing} pixels differ from the oracle in some bit")
    finally:
        orc.close()
        dev.close()


@pytest.mark.parametrize("builder", ["ploc", "lbvh"])
def test_leaf_of_eight_on_tiny_scenes(gpu, sg, builder):
    opts = dict(lbvh_leaf_tris=8, **_builder_opts(gpu, builder))
    sc = _scene(sg, "soup_5")
    dump = _dump_of(gpu, sc, **opts)
    assert dump["root"] == LEAF | 5 << 27 and len(dump["nodes"]) == 0  # the root is a leaf reference with count 5
    check_invariants(dump, sc.positions, max_leaf=8)
    sc = _scene(sg, "soup_9")
    dump = _dump_of(gpu, sc, **opts)
    assert len(dump["nodes"]) == 1 and dump["root"] == 0  # one inner node, leaves of 8 and 1
    assert dump["nodes"][0, 12:14].tolist() == [LEAF | 8 << 27, LEAF | 1 << 27 | 8]
    check_invariants(dump, sc.positions, max_leaf=8)


def test_options_clamp(gpu, sg):
    """lbvh_leaf_tris above 8 is 8, ploc_radius above 32 is 32. PLOC numbers its nodes by an atomic, so trees are compared as structures."""
    sc = _scene(sg, "room_5000")
    for builder in ("ploc", "lbvh"):
        o = _builder_opts(gpu, builder)
        eight = lr.nested(_dump_of(gpu, sc, lbvh_leaf_tris=8, **o))
        assert lr.nested(_dump_of(gpu, sc, lbvh_leaf_tris=100, **o)) == eight
        assert lr.nested(_dump_of(gpu, sc, lbvh_leaf_tris=1, **o)) != eight
    r32 = lr.nested(_dump_of(gpu, sc, ploc_radius=32))
    assert lr.nested(_dump_of(gpu, sc, ploc_radius=1000)) == r32
    assert lr.nested(_dump_of(gpu, sc)) != r32  # the default radius (8) builds another tree: the option is read


def test_wide_tree_ignores_the_leaf_size(gpu, sg):
    """The wide collapse regroups single-triangle leaves itself: lbvh_leaf_tris = 4 gives the wide tree of the default, record for record up to
    the order the records are numbered in (inner children and triangle runs are allocated by atomics)."""
    from test_wide_build import decode

    sc = _scene(sg, "room_5000")
    dumps = []
    for opts in ({}, {"lbvh_leaf_tris": 4}):
        dev = gpu.DeviceScene(sc, device_bvh=True, wide=True, **opts)
        dumps.append(dev.bvh_wide_dump())
        dev.close()
    want, got = dumps
    assert len(got["nodes"]) == len(want["nodes"]) and len(got["tris"]) == len(want["tris"]) == sc.n_triangles
    A, B = decode(got["nodes"]), decode(want["nodes"])
    prim_a, prim_b = got["tris"][:, 9], want["tris"][:, 9]
    stack, seen = [(0, 0)], 0
    while stack:
        a, b = stack.pop()
        seen += 1
        assert np.array_equal(A["p"][a].view(np.uint32), B["p"][b].view(np.uint32)) and np.array_equal(A["e"][a], B["e"][b]), (a, b)
        assert A["imask"][a] == B["imask"][b] and A["tri_mask"][a] == B["tri_mask"][b]
        assert np.array_equal(A["qlo"][a], B["qlo"][b]) and np.array_equal(A["qhi"][a], B["qhi"][b])
        n_inner, n_tri = bin(int(A["imask"][a])).count("1"), bin(int(A["tri_mask"][a])).count("1")
        for r in range(n_inner):
            stack.append((int(A["child_base"][a]) + r, int(B["child_base"][b]) + r))
        ta, tb = int(A["tri_base"][a]), int(B["tri_base"][b])
        assert np.array_equal(prim_a[ta : ta + n_tri], prim_b[tb : tb + n_tri])
    assert seen == len(want["nodes"])


# ---- e. outside the fast-division range ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["ploc", "lbvh"])
def test_device_build_outside_fast_division_range(gpu, oracle, sg, builder):
    """The tiny_box_coordinate scene of tests/test_gpu_parity.py (one coordinate is 1e-13: the per-scene guarantee of the fast node step is void)
    built ON THE DEVICE: k_leaves raises fast_bad, the scene takes the exact path, and hits and image are the oracle's."""
    sc = sg.room_scene(300, seed=41, n_lights=3, n_materials=5, tex_size=8, n_tex_sets=2)
    sc.positions = sc.positions.copy()
    sc.positions[20, 0, 1] = np.float32(1e-13)
    orc = oracle.OracleScene(sc)
    dev = gpu.DeviceScene(sc, device_bvh=True, **_builder_opts(gpu, builder))
    try:
        check_invariants(dev.bvh_device_dump(0), sc.positions, max_leaf=1)
        ties = compare_hits_with_oracle(orc, dev, random_rays(sc, 20_000, seed=12), max_tie_share=NO_MORE_TIES_THAN)
        differing = _render_contract(orc, dev, 40, 32, 4, f"tiny_box_coordinate, {builder}")
        print(f"\n[tiny_box_coordinate, {builder}] tie share {ties:.2e}, {differing} pixels differ from the oracle in some bit")
    finally:
        orc.close()
        dev.close()


# ---- f. the second trip of the grid-stride loops ---------------------------------------------------------------------------------------------
def test_grid_stride_loops_take_a_second_trip(gpu, sg):
    """4096 blocks x 256 threads + 257 triangles, one per leaf: the smallest build in which a thread of k_bounds, k_keys, k_leaves, k_radix_tree
    and k_refit loops twice (257 threads of the first two blocks do). Order, tree and every stored box, all on arrays."""
    t0 = time.perf_counter()
    n = 4096 * 256 + 257
    rng = np.random.default_rng(2)
    pos = (rng.uniform(0.0, 100.0, size=(n, 1, 3)) + rng.uniform(-0.05, 0.05, size=(n, 3, 3))).astype(np.float32)
    sc = _soup_scene(sg, pos, sg.look_camera((50.0, 50.0, 160.0), yaw_deg=0.0, yfov=0.9))
    t1 = time.perf_counter()
    dev = gpu.DeviceScene(sc, device_bvh=True, device_builder=gpu.RT_BUILDER_LBVH, lbvh_leaf_tris=1)
    try:
        dump = dev.bvh_device_dump(0)
        build_ms = dev.build_times()["build_ms"]
    finally:
        dev.close()
    t2 = time.perf_counter()
    walk, k64 = _assert_radix_tree(dump, pos, 1)  # (a) and (b)
    assert len(np.unique(k64 >> np.uint64(32))) < n  # some keys repeat: the stable order and the index half of the keys matter
    want = lr.child_boxes(dump, walk, pos)
    got = dump["nodes"][:, 0:12]
    bad = np.nonzero((got != want.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, f"{len(bad)} inner nodes store a child box that is not the exact box of the child's range, first: node {bad[0]}"
    assert walk["height"] <= 62
    # leaf flags of single-triangle leaves, and the records themselves
    tris = dump["tris"]
    assert (tris[:, 10] == 3).all()
    v = pos[tris[:, 9]]
    assert np.array_equal(tris[:, 0:3], v[:, 0].view(np.uint32)) and np.array_equal(tris[:, 3:6], (v[:, 1] - v[:, 0]).view(np.uint32))
    assert np.array_equal(tris[:, 6:9], (v[:, 2] - v[:, 0]).view(np.uint32))
    t3 = time.perf_counter()
    print(f"\n[second trip] {n} triangles: scene {t1 - t0:.1f} s, create + dump {t2 - t1:.1f} s (device build {build_ms:.1f} ms), checks {t3 - t2:.1f} s, "
          f"height {walk['height']}; {t3 - t0:.1f} s in all")
