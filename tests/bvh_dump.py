"""The binary BVH as it sits in HBM (DeviceScene.bvh_device_dump: DevNode / DevTri records, DESIGN.md 'Data layout in HBM'), restated in numpy.

A plain module next to the tests. `flatten_reference` turns a reference-style node list (bvh_info) into those records: tests/test_gpu_bvh_device.py
compares it with what a host-built scene holds in HBM, tests/test_walk_census.py feeds it to deep_walks.dump_census.

A child reference (words 12 and 13 of a node record, and the root) is an inner-node index, or LEAF | count << 27 | first triangle record for a
leaf of 1..8 triangles (count 0: the leaf ends at the record whose flag word, word 10, has bit 0 set).

`check_invariants` and `compare_hits_with_oracle` are what every device-built binary tree is held to, whatever its topology
(tests/test_gpu_bvh_device.py, tests/test_gpu_device_builders.py)."""
import numpy as np

from hit_contract import summary, verify_hits

LEAF = 0x80000000
MASK = 0x07FFFFFF
NONE = 0xFFFFFFFF


def flatten_reference(info, positions):
    """numpy restatement of the DevNode / DevTri layout (DESIGN.md 'Data layout in HBM') from rt_bvh_info's node list."""
    nodes, order = info["nodes"], info["order"]
    inner = nodes[:, 6] != 0xFFFFFFFF
    dev_index = np.cumsum(inner) - 1

    def ref(i):
        if inner[i]:
            return int(dev_index[i])
        b, e = int(nodes[i, 8]), int(nodes[i, 9])
        cnt = e - b
        return LEAF | ((cnt << 27) if 1 <= cnt <= 8 else 0) | b

    out = np.zeros((int(inner.sum()), 16), dtype=np.uint32)
    for i in np.nonzero(inner)[0]:
        l, r = int(nodes[i, 6]), int(nodes[i, 7])
        out[dev_index[i], 0:6] = nodes[l, 0:6]
        out[dev_index[i], 6:12] = nodes[r, 0:6]
        out[dev_index[i], 12] = ref(l)
        out[dev_index[i], 13] = ref(r)
    p = positions[order].astype(np.float32)
    tris = np.zeros((len(order), 12), dtype=np.uint32)
    tris[:, 0:3] = p[:, 0].view(np.uint32)
    tris[:, 3:6] = (p[:, 1] - p[:, 0]).astype(np.float32).view(np.uint32)
    tris[:, 6:9] = (p[:, 2] - p[:, 0]).astype(np.float32).view(np.uint32)
    tris[:, 9] = order
    leaves = nodes[~inner]
    leaves = leaves[leaves[:, 9] > leaves[:, 8]]
    tris[leaves[:, 9] - 1, 10] |= 1
    tris[leaves[:, 8], 10] |= 2
    return out, tris, ref(info["root"]) if info["root"] != 0xFFFFFFFF else 0xFFFFFFFF


def check_invariants(dump, positions, max_leaf):
    """A device-built binary tree is a proper BVH over all triangles: the records are a permutation of the triangles and hold their operands
    bit for bit, every inner record is reached once, every leaf holds 1..max_leaf records and is flagged at both ends, every triangle is in
    exactly one leaf, every stored child box is the exact box of its subtree, and no path is deeper than the traversal stacks. Returns the depth."""
    nodes, tris, root = dump["nodes"], dump["tris"], dump["root"]
    n = tris.shape[0]
    assert sorted(tris[:, 9].tolist()) == list(range(n)), "leaf order is not a permutation of the triangles"
    verts = positions[tris[:, 9]].astype(np.float32)  # original vertices, in leaf order
    # words 0..8 of a DevTri record: a, b - a, c - a of the triangle it names, each difference rounded once
    assert np.array_equal(tris[:, 0:3], verts[:, 0].view(np.uint32)), "DevTri.a is not the triangle's first vertex"
    assert np.array_equal(tris[:, 3:6], (verts[:, 1] - verts[:, 0]).astype(np.float32).view(np.uint32)), "DevTri.v is not float32(b - a)"
    assert np.array_equal(tris[:, 6:9], (verts[:, 2] - verts[:, 0]).astype(np.float32).view(np.uint32)), "DevTri.u is not float32(c - a)"
    tlo, thi = verts.min(axis=1), verts.max(axis=1)
    covered = np.zeros(n, dtype=np.int32)
    f32 = lambda w: w.view(np.float32)  # noqa: E731
    # iterative post-order: box of every subtree from the triangles, compared with the box stored in the parent
    stack = [(root, 0, None)]  # (ref, depth, where the parent stores this child's box)
    boxes = {}
    order = []
    max_depth = 0
    while stack:
        ref, depth, _ = stack.pop()
        max_depth = max(max_depth, depth)
        order.append(ref)
        if ref & LEAF:
            continue
        stack.append((int(nodes[ref, 12]), depth + 1, None))
        stack.append((int(nodes[ref, 13]), depth + 1, None))
    visited_inner = [r for r in order if not (r & LEAF)]
    assert len(set(visited_inner)) == len(visited_inner) == nodes.shape[0], "inner nodes are not a tree over all records"
    for ref in reversed(order):
        if ref & LEAF:
            b, cnt = ref & MASK, (ref >> 27) & 15
            assert 1 <= cnt <= max_leaf
            covered[b : b + cnt] += 1
            assert tris[b, 10] & 2 and tris[b + cnt - 1, 10] & 1
            boxes[ref] = (tlo[b : b + cnt].min(axis=0), thi[b : b + cnt].max(axis=0))
        else:
            l, r = int(nodes[ref, 12]), int(nodes[ref, 13])
            (llo, lhi), (rlo, rhi) = boxes[l], boxes[r]
            assert np.array_equal(f32(nodes[ref, 0:3]), llo) and np.array_equal(f32(nodes[ref, 3:6]), lhi), ref
            assert np.array_equal(f32(nodes[ref, 6:9]), rlo) and np.array_equal(f32(nodes[ref, 9:12]), rhi), ref
            boxes[ref] = (np.minimum(llo, rlo), np.maximum(lhi, rhi))
            del boxes[l], boxes[r]
    assert (covered == 1).all(), "a triangle is in no leaf or in two"
    assert max_depth <= 62
    return max_depth


def compare_hits_with_oracle(orc, dev, rays, max_tie_share, brute="all"):
    """Closest hits of a device-built tree against the oracle's: t bit-equal on every ray, same hit / miss; where the index agrees
    the barycentrics are bit-equal too; where it differs the two triangles tie exactly in t (asserted by the first check), and the returned
    triangle's own test gives the returned (b, c, t) bit for bit (hit_contract.verify_hits, kind "exact")."""
    op, ob = orc.cast_rays(rays)
    gp, gb = dev.cast_rays(rays)
    assert np.array_equal(op == 0xFFFFFFFF, gp == 0xFFFFFFFF)
    bad = ob[:, 2].view(np.uint32) != gb[:, 2].view(np.uint32)
    assert not bad.any(), f"closest-hit distance differs from the oracle on {int(bad.sum())} of {len(rays)} rays"
    same = op == gp
    assert np.array_equal(gb[same].view(np.uint32), ob[same].view(np.uint32))
    share = float(1 - same.mean())
    assert share <= max_tie_share, f"{int((~same).sum())} index mismatches (exact ties) of {len(rays)} rays: more than {max_tie_share:.1e}"
    c = verify_hits(orc, rays, op, ob, gp, gb, "exact", brute=brute)
    print(f"\ndevice-built tree: {summary(c)}")
    assert c["ties"] == int((~same).sum())
    return share
