"""OracleScene.walk_census (oracle/rt_oracle.cpp rto_walk_census) on a tree small enough to walk by hand. CPU only.

The census says how many deferred far siblings each of the oracle's two recursions holds at once; tests/test_gpu_deep_walks.py uses it to
prove that its rays reach the slow tiers of the device's traversal stacks. Here the expected counts are written out.

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
