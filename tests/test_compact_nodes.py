"""The compact node records of the binary tree (csrc/rt_device_types.h DevNodeCompact, compact_derive_node), without a GPU.

rt_compact_derive_host runs the function the device kernel runs, on host arrays. The trees are the reference-topology host builds of the
600-triangle golden scenes and of a 4 096-triangle room, flattened into DevNode records by tests/bvh_dump.py. For every inner child with
`valid`, (the parent's box of the child, the compact record, the six selector bits) expand into the child's own record, all 14 words, bit for
bit; every leaf child has valid = 0; and a box looser than the union of its children's costs exactly the affected child its `valid`."""
import numpy as np
import pytest

from bvh_dump import LEAF, flatten_reference
from conftest import golden_scene_specs, make_scene

VALID = 0x40


def expand(nodes, compact):
    """Per (node, side): `valid`, and the child's record as wf_extend rebuilds it from the parent's box, the compact record and the selectors."""
    out = {}
    for i, row in enumerate(nodes):
        for side in (0, 1):
            s = (int(row[14]) >> (8 * side)) & 0x7F
            c = int(row[12 + side])
            if not s & VALID:
                out[(i, side)] = None
                continue
            assert not c & LEAF, f"node {i} side {side}: a leaf child has valid"
            box, p = row[6 * side : 6 * side + 6], compact[c]
            rec = np.zeros(14, dtype=np.uint32)
            for f in range(6):
                rec[f], rec[6 + f] = (p[f], box[f]) if (s >> f) & 1 else (box[f], p[f])
            rec[12:14] = p[6:8]
            out[(i, side)] = (c, rec)
    return out


def flat_tree(rt, sc):
    nodes, _, _ = flatten_reference(rt.bvh_build_host(sc.positions), sc.positions.reshape(-1, 3, 3))
    return nodes


def room4096(sg):
    return sg.room_scene(4096, seed=5, n_lights=4, n_materials=6, tex_size=0)


def check_tree(rt, nodes):
    derived, compact = rt.compact_derive_host(nodes)
    assert np.array_equal(derived[:, :14], nodes[:, :14]) and np.array_equal(derived[:, 15], nodes[:, 15]), "the derivation writes word 14 alone"
    n_valid = 0
    for (i, side), e in expand(derived, compact).items():
        c = int(nodes[i, 12 + side])
        if c & LEAF:
            assert e is None, f"node {i} side {side}: leaf child with valid = 1"
        elif e is not None:
            assert np.array_equal(e[1], nodes[c, :14]), f"node {i} side {side}: child {c} expands to {e[1]}, its record is {nodes[c, :14]}"
            n_valid += 1
    return derived, compact, n_valid


@pytest.mark.parametrize("name", list(golden_scene_specs()) + ["room4096"])
def test_valid_children_expand_to_their_records_bit_for_bit(rt, sg, name):
    sc = room4096(sg) if name == "room4096" else make_scene(sg, golden_scene_specs()[name])
    nodes = flat_tree(rt, sc)
    _, compact, n_valid = check_tree(rt, nodes)
    inner_children = int(((nodes[:, 12:14] & LEAF) == 0).sum())
    assert inner_children == len(nodes) - 1 and n_valid == inner_children, "the host builder makes every box the exact union of its children's"
    root = sorted(set(range(len(nodes))) - set(int(c) for c in nodes[:, 12:14].ravel() if not c & LEAF))
    assert len(root) == 1 and not compact[root[0]].any(), "the root's slot is never written"


def test_a_looser_box_costs_the_affected_child_its_valid_bit(rt, sg):
    """Node N's box of an inner child C moved outwards on one face, each face in turn: neither of C's children has that plane any more, so
    C, and only C, loses `valid`."""
    nodes = flat_tree(rt, room4096(sg))
    base, _, n_base = check_tree(rt, nodes)
    # N = the root: nobody holds a box of the root, so the planes that move are compared once only (any other N would lose its own valid too)
    i = (set(range(len(nodes))) - set(int(c) for c in nodes[:, 12:14].ravel() if not c & LEAF)).pop()
    side = 0 if not nodes[i, 12] & LEAF else 1
    assert not nodes[i, 12 + side] & LEAF
    for f in range(6):
        loose = nodes.copy()
        w = loose[i, 6 * side + f : 6 * side + f + 1].view(np.float32)
        w[0] = w[0] - 1.0 if f < 3 else w[0] + 1.0
        derived, _, n_valid = check_tree(rt, loose)
        assert ((int(derived[i, 14]) >> (8 * side)) & VALID) == 0, f"face {f}: the child of a looser box kept valid"
        assert n_valid == n_base - 1
        other = derived[:, 14].copy()
        other[i] = (other[i] & ~np.uint32(0x7F << (8 * side))) | (base[i, 14] & np.uint32(0x7F << (8 * side)))
        assert np.array_equal(other, base[:, 14]), f"face {f}: another child's bits changed"


def test_nan_and_negative_zero_planes_compare_by_bits(rt):
    """The comparison is of bits: -0.0 is not +0.0 (the rebuilt record would differ in a bit), and a NaN plane equals itself."""
    f = lambda *v: np.array(v, dtype=np.float32).view(np.uint32)  # noqa: E731
    nodes = np.zeros((2, 16), dtype=np.uint32)
    nodes[0, 0:6], nodes[0, 6:12] = f(0.0, 0.0, 0.0, 1.0, 1.0, np.nan), f(2.0, 2.0, 2.0, 3.0, 3.0, 3.0)
    nodes[0, 12:14] = (1, LEAF | (1 << 27))
    nodes[1, 0:6], nodes[1, 6:12] = f(0.0, 0.0, 0.0, 0.5, 1.0, np.nan), f(0.25, 0.5, 0.5, 1.0, 0.75, 0.5)
    nodes[1, 12:14] = (LEAF | (1 << 27) | 1, LEAF | (1 << 27) | 2)
    check_tree(rt, nodes)
    derived, _ = rt.compact_derive_host(nodes)
    assert int(derived[0, 14]) & VALID
    nodes[1, 0] = f(-0.0)[0]
    derived, _ = rt.compact_derive_host(nodes)
    assert not int(derived[0, 14]) & VALID
