"""tests/lbvh_replay.py against brute force, on the CPU: hand-made Morton keys, the radix tree's definition against the property that defines a
radix tree (every node is a maximal set of leaves sharing a prefix), the array version against the plain one, and the condition the GPU test
of PLOC rests on: the replayed rounds build the largest-gap tree of a ruler scene, for every radius, without a forced round."""
import numpy as np
import pytest

import lbvh_replay as lr
from bvh_dump import LEAF

F32 = np.float32


def _tri_at(c):
    """A triangle with all three vertices at c: its centre is ((c + c) + c) / 3."""
    c = np.asarray(c, dtype=F32)
    return np.stack([c, c, c]).astype(F32)


def test_hand_made_keys():
    lo, hi = (0.0, 0.0, 0.0), (3.0, 6.0, 12.0)
    corner = lambda *bits: tuple(h if b else l for b, l, h in zip(bits, lo, hi))  # noqa: E731
    pos = np.stack([_tri_at(lo), _tri_at(hi), _tri_at(corner(1, 0, 0)), _tri_at(corner(0, 1, 0)), _tri_at(corner(0, 0, 1))])
    keys = lr.morton_keys(pos)
    assert keys[0] == 0  # the low corner
    assert keys[1] == 0x3FFFFFFF  # the high corner: 1024 clamps to 1023 on every axis
    # one axis at its top cell, the others at 0: x on bits 0, 3, ..., y on bits 1, 4, ..., z on bits 2, 5, ...
    assert keys[2] == 0x09249249 and keys[3] == 0x09249249 << 1 and keys[4] == 0x09249249 << 2
    # the middle of the second cell on one axis: bit 0, 1 or 2 of the lowest triple
    step = np.array(hi, dtype=F32) * F32(1.5 / 1024)
    pos2 = np.stack([_tri_at(lo), _tri_at(hi)] + [_tri_at(np.eye(3, dtype=F32)[c] * step) for c in range(3)])
    assert lr.morton_keys(pos2)[2:].tolist() == [1, 2, 4]
    # zero extent on one axis leaves that axis' bits 0
    for c in range(3):
        flat = pos.copy()
        flat[..., c] = F32(0.5)
        k = lr.morton_keys(flat)
        assert not (k & np.uint32(0x09249249 << c)).any() and k[1] == 0x3FFFFFFF & ~(0x09249249 << c)
    assert lr.spread10(np.array([1023, 1, 2, 512])).tolist() == [0x09249249, 1, 8, 1 << 27]


def test_keys_round_in_float32():
    """The centre is (p0 + p1) + p2, then / 3, each rounded to float32: a case where double arithmetic lands in another cell."""
    rng = np.random.default_rng(1)
    pos = rng.uniform(-3, 5, size=(20000, 3, 3)).astype(F32)
    keys = lr.morton_keys(pos)
    lo, hi = lr.scene_bounds(pos)
    ctr = pos.astype(np.float64).sum(axis=1) / 3
    q64 = np.clip((ctr - lo) * (1024.0 / (hi.astype(np.float64) - lo)), 0, 1023).astype(np.uint32)
    k64 = lr.spread10(q64[:, 0]) | lr.spread10(q64[:, 1]) << np.uint32(1) | lr.spread10(q64[:, 2]) << np.uint32(2)
    assert 0 < (keys != k64).sum() < 200  # a few centres sit within a float32 rounding of a cell border; the replay follows the device there
    order = lr.leaf_order(keys)
    assert (np.diff(keys[order].astype(np.int64)) >= 0).all()
    same = np.diff(keys[order].astype(np.int64)) == 0
    assert (np.diff(order)[same] > 0).all()  # stable: equal keys keep index order


def _key_set(n, distinct, seed):
    """n sorted unique 64-bit leaf keys whose upper halves take min(distinct, n) values, each at least once."""
    rng = np.random.default_rng(seed)
    distinct = min(distinct, n)
    values = rng.choice(1 << 30, size=distinct, replace=False)
    upper = np.sort(values[np.concatenate([np.arange(distinct), rng.integers(0, distinct, size=n - distinct)])])
    assert len(np.unique(upper)) == distinct
    return (upper.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)


@pytest.mark.parametrize("n", [2, 3, 257, 1000])
@pytest.mark.parametrize("distinct", [1, 2, 7, "n"])
def test_radix_tree_is_the_prefix_tree(n, distinct):
    keys = _key_set(n, n if distinct == "n" else distinct, seed=n)
    assert (np.diff(keys.astype(object)) > 0).all()
    tree = lr.radix_tree(keys)
    assert sorted(tree) == list(range(n - 1))  # every inner index once
    ik = [int(k) for k in keys]
    leaf_parent, node_parent = {}, {}
    for node, (a, b, g) in tree.items():
        assert a <= g < b
        # node indices as defined: a node's index is one end of its range, the root is 0 over everything
        assert node in (a, b) and (node != 0 or (a, b) == (0, n - 1))
        # the range is exactly the set of leaves sharing the prefix above the first bit in which its ends differ: maximal
        bit = (ik[a] ^ ik[b]).bit_length()
        share = [k for k in range(n) if ik[k] >> bit == ik[a] >> bit]
        assert share == list(range(a, b + 1)), (node, a, b)
        # children partition it: left [a, g] is node g (or leaf g), right [g + 1, b] is node g + 1 (or leaf g + 1)
        for child, (ca, cb) in ((g, (a, g)), (g + 1, (g + 1, b))):
            if ca == cb:
                assert child not in leaf_parent
                leaf_parent[child] = node
            else:
                assert child not in node_parent and tree[child][:2] == (ca, cb)
                node_parent[child] = node
        # the split is where that bit turns from 0 to 1
        assert not (ik[g] >> (bit - 1)) & 1 and (ik[g + 1] >> (bit - 1)) & 1
    assert sorted(leaf_parent) == list(range(n)) and sorted(node_parent) == list(range(1, n - 1))
    first, last, split = lr.radix_tree_arrays(keys)
    assert [tuple(t) for t in np.stack([first, last, split], axis=1).tolist()] == [tree[i] for i in range(n - 1)]


def test_radix_children_references():
    keys = _key_set(10, 10, seed=5)
    first, last, split = lr.radix_tree_arrays(keys)
    left, right = lr.radix_children(first, last, split, n_tris=28, leaf_tris=3)  # 10 leaves, the last holds 1
    refs = np.concatenate([left, right])
    leaves = refs[(refs & LEAF) != 0]
    assert sorted((leaves & 0x07FFFFFF).tolist()) == list(range(0, 30, 3))
    assert sorted(((leaves >> 27) & 15).tolist()) == [1] + [3] * 9
    assert sorted(refs[(refs & LEAF) == 0].tolist()) == list(range(1, 9))


RULERS = [(600, 0), (600, 1), (257, 255), (513, 3), (300, 7)]


@pytest.mark.parametrize("radius", [1, 8, 32])
@pytest.mark.parametrize("n,offset", RULERS)
def test_ploc_replay_builds_the_largest_gap_tree(n, offset, radius):
    pos, x = lr.ruler_positions(n, offset)
    want = lr.largest_gap_tree(x)
    tree, rounds, forced = lr.ploc_replay(lr.triangle_boxes(pos), radius)
    assert tree == want
    assert forced == 0 and rounds <= 12, (rounds, forced)


def test_ploc_replay_on_collapsed_and_scattered_boxes():
    """All boxes equal (every area ties): the pairing partner wins, so a round halves the clusters and pairs (2k, 2k + 1). Scattered boxes: a
    proper tree over all of them, left before right."""
    tree, rounds, forced = lr.ploc_replay(np.tile(np.array([0, 0, 0, 1, 1, 1], dtype=F32), (8, 1)), 8)
    assert tree == (((0, 1), (2, 3)), ((4, 5), (6, 7))) and (rounds, forced) == (3, 0)
    rng = np.random.default_rng(3)
    pos = (rng.uniform(0, 10, size=(300, 1, 3)) + rng.uniform(-0.3, 0.3, size=(300, 3, 3))).astype(F32)
    tree, rounds, forced = lr.ploc_replay(lr.triangle_boxes(pos), 8)
    leaves = []

    def collect(t):
        if isinstance(t, tuple):
            assert len(t) == 2
            collect(t[0])
            collect(t[1])
        else:
            leaves.append(t)

    collect(tree)
    assert sorted(leaves) == list(range(300)) and rounds < 40


def test_largest_gap_tree_refuses_a_tie():
    assert lr.largest_gap_tree([0.0, 1.0, 3.0]) == ((0, 1), 2)
    with pytest.raises(AssertionError):
        lr.largest_gap_tree([0.0, 1.0, 2.0])


def test_walk_binary_on_a_hand_made_dump():
    """((0, 1), (2..3, 4)) with its records numbered out of order."""
    leaf = lambda b, c: LEAF | c << 27 | b  # noqa: E731
    nodes = np.zeros((3, 16), dtype=np.uint32)
    nodes[2, 12:14] = (1, 0)  # root
    nodes[1, 12:14] = (leaf(0, 1), leaf(1, 1))
    nodes[0, 12:14] = (leaf(2, 2), leaf(4, 1))
    dump = dict(root=2, nodes=nodes, tris=np.zeros((5, 12), dtype=np.uint32))
    w = lr.walk_binary(dump)
    assert w["contiguous"] and w["height"] == 2 and [l.tolist() for l in w["levels"]] == [[2], [1, 0]]
    assert (w["lfirst"][2], w["llast"][2], w["rfirst"][2], w["rlast"][2]) == (0, 1, 2, 4) and w["depth"].tolist() == [1, 1, 0]
    assert lr.nested(dump) == ((0, 1), (range(2, 4), 4))
    nodes[0, 13] = 1  # a record reached twice
    with pytest.raises(AssertionError):
        lr.walk_binary(dump)
