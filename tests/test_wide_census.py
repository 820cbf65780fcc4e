"""CPU tests of the census of the 8-wide walk (deep_walks.wide_census: oracle/rt_oracle.cpp rto_wide_census, and its second statement
deep_walks.wide_census_numpy), and of what tests/test_gpu_deep_wide_walks.py relies on. No GPU.

wf_extend_wide keeps the newest pending node group in registers, eight more in an LDS ring and the rest in a global workspace: the 10th
pending group (deep_walks.WIDE_RING_EVICT) is the first eviction. Which rays get there is counted, not assumed, and the counting is held
to hand-worked numbers on a tree of six nodes here. The trees the GPU tests walk are the HOST collapse (bvh_wide_build_host) of two
corner-ladder scenes; their depths (19 and 22 levels) and the share of rays that keep at least 12 groups pending, for rays of one octant and
of all eight, are pinned here, so that a change of the host builder that takes the GPU tests out of the workspace tier is noticed without a
GPU. Measured (4000 rays each; the tests print theirs):

    scene                  wide nodes / levels   corner rays (one octant)    octant rays (all eight)
    2^13 soup, seed 62     835 / 19              14 pending on every ray     12 to 16, every ray >= 12 in every octant
    2^15 soup, seed 62     3336 / 22             17 pending on every ray     15 to 19, every ray >= 12 in every octant
    2^10 soup, seed 61     108 / 10              8 or 9: the ring exactly full, no eviction; all octants: 5 to 9
"""
import numpy as np
import pytest

import deep_walks as dw
from test_wide_build import walk_and_check

N_RAYS = 4000
NINE_IN_TEN = 0.9
CLAIM = {dw.WIDE_CLAIM: NINE_IN_TEN}


# ------------------------------------------------------------------------------------------------ a tree worked by hand
# Every node has the grid origin (0, 0, 0) and cells of 1, so a plane byte IS the coordinate. Triangle T lies in the plane x = X with its
# right angle at (y, z) = (0, 0) and legs along y and z: a ray along x at (y, z) hits it when y / leg_y + z / leg_z <= 1.
#   T0  x = 100, legs 20, 20      T1  x = 60, legs 20, 4      T2, T3, T4  x = 10, 20, 30, legs 20, 20
#   node 0 (root)   slot 0 inner -> node 1, slot 1 inner -> node 2, slot 2 leaf {T0}
#   node 1          slots 0, 1, 2 inner -> nodes 3, 4, 5                                  box x 10..30, y 0..20, z 0..20
#   node 2          slot 0 leaf {T1}                                                      box x 60,     y 0..20, z 0..4
#   nodes 3, 4, 5   slot 0 leaf {T2}, {T3}, {T4}
# Triangle records are in node order (T0, T1, T2, T3, T4); the scene stores the triangles in another order, so `order` is no identity.
HAND_TRIS = {0: (100, 20, 20), 1: (60, 20, 4), 2: (10, 20, 20), 3: (20, 20, 20), 4: (30, 20, 20)}  # record -> (x, leg_y, leg_z)
HAND_ORDER = np.array([3, 0, 4, 1, 2], dtype=np.uint32)  # record k is scene triangle HAND_ORDER[k]


def hand_tree():
    pos = np.zeros((5, 3, 3), dtype=np.float32)
    for k, (x, ly, lz) in HAND_TRIS.items():
        pos[HAND_ORDER[k]] = [[x, 0, 0], [x, ly, 0], [x, 0, lz]]
    box = {k: ((x, 0, 0), (x, ly, lz)) for k, (x, ly, lz) in HAND_TRIS.items()}  # of triangle record k
    node1 = ((10, 0, 0), (30, 20, 20))
    nodes = np.zeros((6, 20), dtype=np.uint32)
    b = nodes.view(np.uint8).reshape(6, 80)

    def fill(i, imask, child_base, tri_base, tri_mask, slots):
        b[i, 12:15] = 127
        b[i, 15] = imask
        nodes[i, 4:7] = child_base, tri_base, tri_mask
        b[i, 32:56], b[i, 56:80] = 255, 0  # empty slots: inverted boxes
        for s, (lo, hi) in slots.items():
            for a in range(3):
                b[i, 32 + 8 * a + s], b[i, 56 + 8 * a + s] = lo[a], hi[a]

    fill(0, 0b011, 1, 0, 0b001 << 6, {0: node1, 1: box[1], 2: box[0]})
    fill(1, 0b111, 3, 1, 0, {0: box[2], 1: box[3], 2: box[4]})
    fill(2, 0, 6, 1, 0b001, {0: box[1]})
    for j in range(3):
        fill(3 + j, 0, 6, 2 + j, 0b001, {0: box[2 + j]})
    return {"nodes": nodes, "order": HAND_ORDER}, pos


# (origin, direction) -> the largest number of groups pending, worked by the rule of deep_walks.wide_census
HAND_RAYS = [
    # +x at (y, z) = (5, 2), octant 0: slot 0 goes first. The root's three slots are hit; T0 is hit at t = 105. Step into node 1, the rest of
    # the root's group (slot 1) is pushed: 1. Node 1's three slots are hit (t = 15, 25, 35 < 105); step into node 3, the rest {1, 2} is pushed
    # as ONE frame: 2. T2 at t = 15. The frame {1, 2} comes back without a test: node 4 (its rest {2} pushed: 2 again) misses [EPS, 15], so
    # do node 5 and, from the root's frame, node 2.
    ((-5, 5, 2), (1, 0, 0), 2),
    # the same at z = 7: above node 2's box (z <= 4). The root's group is slot 0 alone, nothing is pushed for it; node 1's rest is: 1.
    ((-5, 5, 7), (1, 0, 0), 1),
    # -x from x = 200, octant 1: slot 1 goes before slot 0. T0 at t = 100, first. Step into node 2 (t = 140), the rest (slot 0) pushed: 1;
    # nothing of node 2 lies within [EPS, 100]. The frame comes back untested, node 1 is fetched, and none of its boxes (t >= 170) is hit.
    ((200, 5, 2), (-1, 0, 0), 1),
    # +x at (18, 3): inside every box, outside every triangle (18 / 20 + 3 / 20 > 1), so nothing is ever culled and all six nodes are
    # fetched: the root's rest pushed (1), node 1's rest {1, 2} (2), then {2} (2 again), node 2 last.
    ((-5, 18, 3), (1, 0, 0), 2),
    # +x at (15, 15): beyond node 2's box and outside every triangle (15 / 20 + 15 / 20 > 1), so nothing is ever culled: the root's group is
    # slot 0 alone, node 1 pushes {1, 2}, later {2}: 1 throughout.
    ((-5, 15, 15), (1, 0, 0), 1),
    # +x at (50, 50): beside the scene. The root's eight boxes are tested and none is hit: 0.
    ((-5, 50, 50), (1, 0, 0), 0),
    # +y from below at x = 15, z = 5 (two direction components are zero: 1 / d = 2^60 there): the root's slot 0 is hit (node 1: x 10..30),
    # slots 1 and 2 (x = 60, 100) are not; node 1's boxes are flat in x, at 10, 20 and 30: none is hit. Nothing is ever pushed: 0.
    ((15, -5, 5), (0, 1, 0), 0),
]


def test_both_censuses_give_the_hand_worked_counts():
    tree, pos = hand_tree()
    depth, hist = walk_and_check(tree["nodes"], tree["order"], pos.reshape(-1, 9))  # the hand-made records are a well-formed wide tree
    assert depth == 3 and hist == {1: 5}
    rays = np.array([list(o) + list(d) for o, d, _ in HAND_RAYS], dtype=np.float32)
    want = [w for _, _, w in HAND_RAYS]
    assert dw.wide_census(tree, pos, rays).tolist() == want
    assert dw.wide_census_numpy(tree, pos, rays).tolist() == want
    # the same records as a device dump hands them over: the order in word 9 of the triangle records
    dump = {"nodes": tree["nodes"], "tris": np.zeros((5, 12), dtype=np.uint32)}
    dump["tris"][:, 9] = HAND_ORDER
    assert dw.wide_census(dump, pos, rays).tolist() == want


def test_census_refuses_records_that_are_no_tree(oracle):
    tree, pos = hand_tree()
    rays = np.array([[-5, 5, 2, 1, 0, 0]], dtype=np.float32)
    bad = tree["nodes"].copy()
    bad[1, 4] = 40  # node 1's children outside the records
    with pytest.raises(RuntimeError):
        oracle.wide_census(bad, tree["order"], pos, rays)
    bad = tree["nodes"].copy()
    bad[1, 4] = 0  # node 1's first child is the root: a cycle
    with pytest.raises(RuntimeError):
        oracle.wide_census(bad, tree["order"], pos, rays)
    with pytest.raises(RuntimeError):
        oracle.wide_census(tree["nodes"], np.array([3, 0, 9, 1, 2], dtype=np.uint32), pos, rays)  # a record names triangle 9 of 5
    assert oracle.wide_census(np.zeros((0, 20), dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros((0, 9), dtype=np.float32), rays).tolist() == [0]


def test_octant_rays_are_corner_rays_turned_into_every_octant():
    a, b = dw.corner_rays(dw.CORNER_CELL, 64, seed=7), dw.octant_rays(dw.CORNER_CELL, 64, seed=7)
    assert np.array_equal(a[:, :3], b[:, :3]) and np.array_equal(np.abs(a[:, 3:]), np.abs(b[:, 3:]))
    octant = (b[:, 3] < 0) * 1 + (b[:, 4] < 0) * 2 + (b[:, 5] < 0) * 4
    assert np.array_equal(octant, np.arange(64) % 8)


# ------------------------------------------------------------------------------------------------ the trees the GPU tests walk
class HostTree:
    def __init__(self, rt, sg, spec):
        self.name = f"corner ladder, 2^{spec['log2_soup']} soup, host-collapsed wide tree"
        self.sc = dw.corner_ladder_scene(sg, **spec)
        self.tree = rt.bvh_wide_build_host(self.sc.positions)
        self.rays = {"corner rays": dw.corner_rays(dw.CORNER_CELL, N_RAYS, seed=7), "octant rays": dw.octant_rays(dw.CORNER_CELL, N_RAYS, seed=7)}
        self.counts = {k: dw.wide_census(self.tree, self.sc.positions, r) for k, r in self.rays.items()}


@pytest.fixture(scope="module")
def trees(rt, sg):
    return {13: HostTree(rt, sg, dw.CORNER_WIDE), 15: HostTree(rt, sg, dw.CORNER_SECOND)}


def test_cpp_census_is_the_numpy_census_ray_for_ray(trees):
    t = trees[13]
    rays = dw.octant_rays(dw.CORNER_CELL, 256, seed=11)
    a, b = dw.wide_census(t.tree, t.sc.positions, rays), dw.wide_census_numpy(t.tree, t.sc.positions, rays)
    assert np.array_equal(a, b), (int((a != b).sum()), a[a != b][:8].tolist(), b[a != b][:8].tolist())
    assert a.min() >= dw.WIDE_RING_EVICT  # not an agreement about shallow walks


@pytest.mark.parametrize("log2_soup", [13, 15])
def test_host_collapsed_corner_trees_reach_the_workspace_tier(trees, log2_soup):
    """What tests/test_gpu_deep_wide_walks.py builds on: the depth of the host-collapsed tree, and at least 90 % of the corner rays, of the
    octant rays, and of the octant rays of EVERY octant on their own, keep 12 groups pending (two past the first eviction)."""
    t = trees[log2_soup]
    assert t.tree["depth"] == dw.CORNER_WIDE_DEPTH[log2_soup]
    depth, _ = walk_and_check(t.tree["nodes"], t.tree["order"], t.sc.positions.reshape(-1, 9))
    assert depth == t.tree["depth"]
    for kind, counts in t.counts.items():
        dw.require_witnesses(f"{t.name}, {len(t.tree['nodes'])} nodes on {t.tree['depth']} levels, {kind}", counts, CLAIM, tag="deep wide", unit="groups",
                             report=(dw.WIDE_RING_EVICT,))
    counts = t.counts["octant rays"]
    shares = [float((counts[k::8] >= dw.WIDE_CLAIM).mean()) for k in range(8)]
    print(f"[deep wide] {t.name}: share of each octant's rays at >= {dw.WIDE_CLAIM}: " + ", ".join(f"{100 * s:.1f} %" for s in shares)
          + "; most pending per octant: " + ", ".join(str(int(counts[k::8].max())) for k in range(8)))
    assert min(shares) >= NINE_IN_TEN, shares


def test_the_scene_of_the_existing_wide_tests_stays_in_the_ring(rt, sg):
    """The negative finding that makes the new GPU tests necessary: on the host-collapsed tree of CORNER_MAIN (the scene of
    test_wide_tree_collapsed_from_the_deep_radix_tree) no ray keeps 10 groups pending, in any octant: the ring is never full."""
    sc = dw.corner_ladder_scene(sg, **dw.CORNER_MAIN)
    tree = rt.bvh_wide_build_host(sc.positions)
    for kind, rays in (("corner rays", dw.corner_rays(dw.CORNER_CELL, N_RAYS, seed=7)), ("octant rays", dw.octant_rays(dw.CORNER_CELL, N_RAYS, seed=7))):
        counts = dw.wide_census(tree, sc.positions, rays)
        _, most = dw.require_witnesses(f"corner ladder, 2^10 soup, host-collapsed wide tree, {len(tree['nodes'])} nodes on {tree['depth']} levels, {kind}",
                                       counts, {}, tag="deep wide", unit="groups", report=(dw.WIDE_RING_EVICT,))
        assert most < dw.WIDE_RING_EVICT, most
