"""OracleScene.walk_census (oracle/rt_oracle.cpp rto_walk_census) on a tree small enough to walk by hand. CPU only.

The census says how many deferred far siblings each of the oracle's two recursions holds at once; tests/test_gpu_deep_walks.py uses it to
prove that its rays reach the slow tiers of the device's traversal stacks. Here the expected counts are written out. The second half of the
file holds deep_walks.dump_census (the same count for a tree given as the device's records) to walk_census, and the generator of the deep
radix trees of tests/test_gpu_deep_device_trees.py to a numpy restatement of the device's builder.

The scene: 8 clusters of 4 emissive triangles. Cluster k lies in the planes x = 10k, 10k + 0.5, 10k + 1, 10k + 1.5, every triangle
(x, -1, -1), (x, 1, -1), (x, 0, 1): its box is [10k, 10k + 1.5] x [-1, 1] x [-1, 1], and at z = 0 a triangle covers |y| <= 0.5. BVH::build
(bvh.h:268-366) halves the clusters along x three times and stops at the clusters (a node of 4 does not split: both halves would be smaller
than 4), which the first test checks:

    root -+- L -+- LL -+- c0        every triangle is emissive, so the light tree is the same tree
          |     |      +- c1
          |     +- LR -+- c2
          |            +- c3
          +- R -+- RL -+- c4
                |      +- c5
                +- RR -+- c6
                       +- c7
"""
import numpy as np
import pytest

import deep_walks as dw
from bvh_dump import LEAF, flatten_reference
from conftest import random_rays


def cluster_scene(sg):
    pos = []
    for k in range(8):
        for j in range(4):
            x = 10.0 * k + 0.5 * j
            pos.append([[x, -1, -1], [x, 1, -1], [x, 0, 1]])
    pos = np.asarray(pos, dtype=np.float32)
    n = len(pos)
    tan = np.tile(np.array([1, 0, 0], dtype=np.float32), (n, 3, 1))
    mats = [sg.Material(color=(1, 1, 1, 1), emission=(1.0, 1.0, 1.0), emissive_strength=1.0, roughness=1.0, metallic=0.0)]
    return sg.Scene(positions=pos, normals=None, texcoords=np.zeros((n, 3, 2), dtype=np.float32), tangents=tan, material_ids=np.zeros(n, dtype=np.uint32),
                    materials=mats, textures=[], camera=sg.look_camera((35.0, 0.0, 30.0), yaw_deg=0.0, yfov=0.9))


# (origin, direction) -> (closest-hit census, light census), each walked by hand on the tree above
CASES = [
    # along +x through every cluster: root, L and LL each have both boxes hit, the near one first: 3 siblings (R, LR, c1) wait while c0 is tested.
    # The light walk goes left first, which is the same order here.
    ((-5.0, 0.0, 0.0), (1.0, 0.001, 0.002), 3, 3),
    # the same line backwards: the near child is the right one every time (R, RR, c7); the light walk still goes left first and defers R, LR, c1
    ((80.0, 0.0, 0.0), (-1.0, 0.001, 0.002), 3, 3),
    # down through c7's box only: root, R and RR each have ONE child hit: nothing is ever deferred
    ((70.7, 5.0, 0.1), (0.01, -1.0, 0.01), 0, 0),
    # from x = 80 towards -x, climbing y = 0.019 (80 - x): inside |y| <= 1 down to x = 27.4, so it crosses c7 .. c4 and c3, and misses c2, LL.
    # closest hit: root both (near R) 1, R both (near RR) 2, RR both (near c7) 3; c7's last triangle is hit at t = 8.5 and prunes all three.
    # light walk, left first: R waits while L is walked (1); in L only LR is hit, in LR only c3: nothing more. Then R with nothing pending:
    # both children hit, RR waits (1); RL both, c5 waits (2); then RR on its own, both, c7 waits (1). Most at once: 2.
    ((80.0, 0.0, 0.0), (-1.0, 0.019, 0.001), 3, 2),
    # from x = -5 towards +x, climbing y = 0.055 (x + 5): 0.91 at the far side of c1, 1.375 at c2: only c0 and c1. Root and L have one child
    # hit, LL both: 1 in either walk.
    ((-5.0, 0.0, 0.0), (1.0, 0.055, 0.001), 1, 1),
]


@pytest.fixture(scope="module")
def orc(oracle, sg):
    o = oracle.OracleScene(cluster_scene(sg))
    yield o
    o.close()


def test_the_hand_tree_is_the_tree_the_docstring_draws(orc):
    NONE = 0xFFFFFFFF
    for which in (0, 1):
        b = orc.bvh_info(which)
        nodes, order = b["nodes"], b["order"]
        assert len(nodes) == 15 and np.array_equal(order, np.arange(32))

        def shape(i):  # nested tuples of leaf ranges
            left, right, begin, end = (int(v) for v in nodes[i, 6:10])
            return (begin, end) if left == NONE else (shape(left), shape(right))

        c = [(4 * k, 4 * k + 4) for k in range(8)]
        assert shape(b["root"]) == (((c[0], c[1]), (c[2], c[3])), ((c[4], c[5]), (c[6], c[7])))


def test_walk_census_counts_written_out_by_hand(orc):
    rays = np.array([list(o) + list(d) for o, d, _, _ in CASES], dtype=np.float32)
    closest, light = orc.walk_census(rays)
    assert closest.tolist() == [c for _, _, c, _ in CASES]
    assert light.tolist() == [l for _, _, _, l in CASES]
    # the rays do what the comments say: all but the third hit a triangle, the first and the last c0's first (index 0), the others c7's last (31)
    prim, bct = orc.cast_rays(rays)
    assert prim.tolist() == [0, 31, 0xFFFFFFFF, 31, 0]
    assert bct[3, 2] == pytest.approx(8.5, rel=1e-3)


def test_walk_census_changes_no_oracle_result_and_no_counter(orc, rt):
    """The census runs the same recursions with a flag set: hits, pdf values and a render's event counters are the same before and after,
    and the same as with many rays (the census splits large batches over threads)."""
    rng = np.random.default_rng(4)
    o = rng.uniform([-5, -2, -2], [80, 2, 2], size=(3000, 3))
    d = rng.normal(size=(3000, 3)) * [1.0, 0.05, 0.05]
    rays = np.concatenate([o, d], axis=1).astype(np.float32)
    before = (orc.cast_rays(rays), orc.light_pdf(rays), orc.run_raytracer(24, 16, 2, seed=3))
    closest, light = orc.walk_census(rays)
    after = (orc.cast_rays(rays), orc.light_pdf(rays), orc.run_raytracer(24, 16, 2, seed=3))
    assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1].view(np.uint32), after[0][1].view(np.uint32))
    assert np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    assert np.array_equal(before[2][0].view(np.uint32), after[2][0].view(np.uint32))
    assert {k: v for k, v in before[2][1].items() if not k.endswith("_ms")} == {k: v for k, v in after[2][1].items() if not k.endswith("_ms")}
    assert closest.max() == 3 and light.max() == 3 and closest.min() == 0  # a tree of 4 levels defers at most 3
    one_by_one = [orc.walk_census(rays[i : i + 1]) for i in range(0, 3000, 97)]
    assert [int(c[0]) for c, _ in one_by_one] == closest[::97].tolist() and [int(l[0]) for _, l in one_by_one] == light[::97].tolist()


# ------------------------------------------------------------------------------------------------ the census of a tree given as device records
FLATTENED = ["room_plain", "boxes", "needles_2000"]


@pytest.mark.parametrize("name", FLATTENED)
def test_dump_census_is_walk_census_on_the_flattened_reference_tree(oracle, sg, scenes, name):
    """deep_walks.dump_census walks DevNode / DevTri records (a device scene's bvh_device_dump). Fed the oracle's own tree, flattened into
    those records, it must count what the oracle's recursion counts, on every ray: multi-triangle leaves, leaves longer than the reference
    field holds, pruning by a hit in the near subtree and axis-parallel rays (infinite and NaN slabs) are all in these three scenes. The numpy
    restatement of the rule agrees on the first 1000 rays."""
    sc = dw.needle_soup_scene(sg, 2000, seed=41) if name == "needles_2000" else scenes[name]
    orc = oracle.OracleScene(sc)
    try:
        nodes, tris, root = flatten_reference(orc.bvh_info(0), sc.positions)
        dump = {"root": root, "nodes": nodes, "tris": tris}
        rays = np.concatenate([random_rays(sc, 6000, seed=3), dw.light_query_rays(sc, 2000, seed=4)])
        want, _ = orc.walk_census(rays)
        got = dw.dump_census(dump, rays)
        assert np.array_equal(got, want), f"{int((got != want).sum())} of {len(rays)} rays"
        assert np.array_equal(dw.dump_census_numpy(dump, rays[:1000]), want[:1000])
        assert want.max() >= (10 if name == "needles_2000" else 5)  # the walks defer and prune: not a census of zeros
        assert dw.dump_depth(dump) >= 8
    finally:
        orc.close()


def test_dump_census_rejects_records_that_are_no_tree(oracle):
    nodes = np.zeros((1, 16), dtype=np.uint32)
    nodes[0, 0:3] = nodes[0, 6:9] = np.array([-1, -1, -1], dtype=np.float32).view(np.uint32)
    nodes[0, 3:6] = nodes[0, 9:12] = np.array([1, 1, 1], dtype=np.float32).view(np.uint32)
    tris = np.zeros((1, 12), dtype=np.uint32)
    tris[0, 10] = 3
    ray = np.array([[0, 0, -3, 0, 0, 1]], dtype=np.float32)
    for left, right in ((0, LEAF | (1 << 27)), (LEAF | (1 << 27) | 5, LEAF | (1 << 27)), (7, LEAF | (1 << 27))):  # a cycle, a triangle and a node out of range
        nodes[0, 12], nodes[0, 13] = left, right
        with pytest.raises(RuntimeError, match="rto_dump_census"):
            dw.dump_census({"root": 0, "nodes": nodes, "tris": tris}, ray)
    nodes[0, 12] = nodes[0, 13] = LEAF | (1 << 27)
    assert dw.dump_census({"root": 0, "nodes": nodes, "tris": tris}, ray).tolist() == [1]


# ------------------------------------------------------------------------------------------------ the scene that makes the radix tree deep
@pytest.mark.parametrize("which", ["main", "second"])
def test_corner_ladder_scene_makes_the_predicted_radix_tree(sg, which):
    """deep_walks.corner_ladder_scene against the numpy restatement of the device's radix builder (morton_keys, radix_tree_dump): the codes are
    what the construction promises, the tree is 31 + log2_soup deep, and the corner rays keep the pending counts the GPU tests of
    tests/test_gpu_deep_device_trees.py require of the device's own tree. A generator that drifts fails here, without a GPU."""
    spec, n_rays, need = (dw.CORNER_MAIN, 20000, {36: 0.9}) if which == "main" else (dw.CORNER_SECOND, 4000, {40: 0.9})
    sc = dw.corner_ladder_scene(sg, **spec)
    n_soup = 2 ** spec["log2_soup"]
    assert sc.n_triangles == n_soup + 32
    pos = sc.positions
    nz = np.abs(pos[pos != 0])
    assert (pos >= 0).all() and nz.min() >= 2.0 ** -37 and nz.max() <= 2.0 ** 40  # 0 or inside the fast-division range
    assert np.array_equal(pos.reshape(-1, 3).min(axis=0), np.zeros(3, dtype=np.float32))
    codes = dw.morton_keys(pos)
    assert (codes[: n_soup + 1] == 0).all()  # the soup and the corner pin: one cell
    assert codes[n_soup + 1] == codes.max() and (codes[n_soup + 1] >> 27) == 7  # the far pin: bit 9 of every axis
    ladder = codes[n_soup + 2 :]
    assert [int(c).bit_length() - 1 for c in ladder] == list(range(30))  # bit b of axis a is the highest of triangle 3 b + a
    box_lo = pos[n_soup + 2 :].min(axis=1)
    assert (box_lo == 0).all()  # every ladder box starts at the corner
    tree = dw.radix_tree_dump(pos)
    assert np.array_equal(tree["order"], np.argsort(codes, kind="stable"))
    assert dw.dump_depth(tree) == dw.CORNER_DEPTH[spec["log2_soup"]] == 31 + spec["log2_soup"]
    rays = dw.corner_rays(dw.CORNER_CELL, n_rays, seed=7)
    d = rays[:, 3:]
    assert (d >= 0.2).all() and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6)
    counts = dw.dump_census(tree, rays)
    dw.require_witnesses(f"corner ladder, 2^{spec['log2_soup']} soup, restated radix tree", counts, need)
    assert counts.max() <= dw.CORNER_DEPTH[spec["log2_soup"]] - 1
    if which == "main":  # the restated rule on the restated tree, for a sample
        assert np.array_equal(dw.dump_census_numpy(tree, rays[:200]), counts[:200])
