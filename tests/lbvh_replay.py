"""The device BVH builders (csrc/rt_bvh_device.hip; PLOC: csrc/rt_bvh_ploc.hip) restated from their definitions, in plain numpy; no GPU.

What a device build computes before any tree exists is a pure function of the float32 input, so it is held exactly:
  * morton_keys: k_bounds + k_keys statement by statement in float32 (every statement rounds once; nothing in it can contract into an FMA and the
    device divides correctly rounded);
  * leaf_order: the stable sort of those keys (rocPRIM's radix sort is stable);
  * radix_tree: the Karras 2012 tree over the 64-bit leaf keys by its top-down DEFINITION (k_radix_tree finds the same tree bottom-up, every node
    on its own); radix_tree_arrays is the same definition level by level on arrays, for a million leaves;
  * largest_gap_tree / ruler_scene / ploc_replay: an input family on which PLOC's result is known by construction, and the rounds of
    k_ploc_nn / k_ploc_merge / k_ploc_compact in Python to show that on the CPU;
  * walk_binary: a bvh_device_dump as the structure those definitions are compared with.
tests/test_lbvh_replay.py checks this module against brute force; tests/test_gpu_device_builders.py compares the device with it."""
import numpy as np

from bvh_dump import LEAF, MASK

F32 = np.float32


# ---- keys and leaf order ---------------------------------------------------------------------------------------------------------------------
def spread10(v):
    """Bit b of the 10-bit v goes to bit 3 b. A loop over the bits, on purpose: the kernel's magic masks are what this checks."""
    v = np.asarray(v, dtype=np.uint32)
    out = np.zeros_like(v)
    for b in range(10):
        out |= ((v >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b)
    return out


def scene_bounds(positions):
    p = np.asarray(positions, dtype=F32).reshape(-1, 3)
    return p.min(axis=0), p.max(axis=0)


def morton_cells(positions):
    """(n, 3) uint32: the 10-bit cell of every triangle's centre on each axis, as k_keys quantises it."""
    p = np.asarray(positions, dtype=F32).reshape(-1, 3, 3)
    lo, hi = scene_bounds(p)
    ext = (hi - lo).astype(F32)
    inv = np.zeros(3, dtype=F32)
    for c in range(3):
        if ext[c] > F32(0):
            inv[c] = F32(1024) / ext[c]
    ctr = (((p[:, 0] + p[:, 1]).astype(F32) + p[:, 2]).astype(F32) / F32(3)).astype(F32)
    s = ((ctr - lo).astype(F32) * inv).astype(F32)
    return np.minimum(np.maximum(s, F32(0)), F32(1023)).astype(np.uint32), inv


def morton_keys(positions):
    """(n,) uint32: the 30-bit Morton key of every triangle, x on bits 0, 3, ..., y on bits 1, 4, ..., z on bits 2, 5, ..."""
    q, _ = morton_cells(positions)
    return spread10(q[:, 0]) | (spread10(q[:, 1]) << np.uint32(1)) | (spread10(q[:, 2]) << np.uint32(2))


def leaf_order(keys):
    return np.argsort(np.asarray(keys), kind="stable")


def leaf_keys64(sorted_keys, leaf_tris):
    """k_leaves: key of the leaf's first triangle << 32 | leaf index. Sorted and unique by construction."""
    first = np.asarray(sorted_keys, dtype=np.uint64)[:: int(leaf_tris)]
    return (first << np.uint64(32)) | np.arange(len(first), dtype=np.uint64)


# ---- the radix tree, by definition -----------------------------------------------------------------------------------------------------------
def _top_bit(x):
    """63 - clz(x) for python ints > 0."""
    return int(x).bit_length() - 1


def radix_tree(keys64):
    """{inner node index: (first, last, split)} over sorted unique 64-bit keys: the range [a, b], a < b, splits after gamma, the last index in
    [a, b) whose key has a 0 at the highest bit in which key[a] and key[b] differ. The root is inner node 0; the left child covers [a, gamma] and
    is inner node gamma (leaf gamma when a == gamma), the right child covers [gamma + 1, b] and is inner node gamma + 1 (leaf when gamma + 1 == b)."""
    keys = [int(k) for k in keys64]
    n = len(keys)
    out = {}
    if n < 2:
        return out
    todo = [(0, 0, n - 1)]
    while todo:
        node, a, b = todo.pop()
        bit = _top_bit(keys[a] ^ keys[b])
        gamma = max(k for k in range(a, b) if not (keys[k] >> bit) & 1)
        assert node not in out
        out[node] = (a, b, gamma)
        if a < gamma:
            todo.append((gamma, a, gamma))
        if gamma + 1 < b:
            todo.append((gamma + 1, gamma + 1, b))
    return out


def _top_bit_u64(x):
    x = x.copy()
    pos = np.zeros(len(x), dtype=np.uint64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (x >> np.uint64(s)) != 0
        pos += np.where(big, np.uint64(s), np.uint64(0))
        x = np.where(big, x >> np.uint64(s), x)
    return pos


def radix_tree_arrays(keys64):
    """radix_tree level by level on arrays: (first, last, split), each (n - 1,) int64 indexed by inner node. Every inner index 0 .. n - 2 is
    reached exactly once (asserted)."""
    keys = np.asarray(keys64, dtype=np.uint64)
    n = len(keys)
    first, last, split = (np.full(max(n - 1, 0), -1, dtype=np.int64) for _ in range(3))
    node, a, b = np.zeros(1, np.int64), np.zeros(1, np.int64), np.full(1, n - 1, np.int64)
    if n < 2:
        return first, last, split
    done = 0
    while len(node):
        bit = _top_bit_u64(keys[a] ^ keys[b])
        # sorted keys sharing every bit above `bit`: the ones with a 0 there come first; the first with a 1 is the first >= prefix : 1 : 0...0
        thr = ((keys[a] >> bit) | np.uint64(1)) << bit
        gamma = np.searchsorted(keys, thr, side="left").astype(np.int64) - 1
        assert (gamma >= a).all() and (gamma < b).all()
        assert (first[node] == -1).all() and len(np.unique(node)) == len(node)
        first[node], last[node], split[node] = a, b, gamma
        done += len(node)
        l, r = a < gamma, gamma + 1 < b
        node, a, b = np.concatenate([gamma[l], gamma[r] + 1]), np.concatenate([a[l], gamma[r] + 1]), np.concatenate([gamma[l], b[r]])
    assert done == n - 1
    return first, last, split


def radix_children(first, last, split, n_tris, leaf_tris):
    """The child references (words 12 and 13 of the DevNode records) k_radix_tree writes for that tree: an inner index, or
    LEAF | count << 27 | first record of a leaf of `leaf_tris` triangles (the last leaf: what is left)."""
    L = int(leaf_tris)

    def leaf_ref(leaf):
        k0 = leaf * L
        return (LEAF | (np.minimum(L, n_tris - k0) << 27) | k0).astype(np.uint32)

    left = np.where(first == split, leaf_ref(split), split.astype(np.uint32))
    right = np.where(split + 1 == last, leaf_ref(split + 1), (split + 1).astype(np.uint32))
    return left.astype(np.uint32), right.astype(np.uint32)


# ---- PLOC on an input whose tree is known -------------------------------------------------------------------------------------------------------
def largest_gap_tree(x):
    """Nested (left, right) tuples over the indices of the ascending x: [a, b] splits at its largest gap x[k + 1] - x[k], which must be unique."""
    x = np.asarray(x, dtype=np.float64)
    gaps = np.diff(x)

    def build(a, b):
        if a == b:
            return a
        g = gaps[a:b]
        k = int(np.argmax(g))
        assert (g == g[k]).sum() == 1, f"the largest gap of [{a}, {b}] is not unique"
        return (build(a, a + k), build(a + k + 1, b))

    return build(0, len(x) - 1)


def ruler_x(n, offset):
    """x of the n triangles: the gap after triangle i is 4 ** ctz(i + offset + 1), from x = 0."""
    i = np.arange(n - 1, dtype=np.int64) + offset + 1
    ctz = np.array([(int(v) & -int(v)).bit_length() - 1 for v in i], dtype=np.int64)
    x = np.concatenate([[0.0], np.cumsum(4.0 ** ctz)])
    assert x.max() < 2 ** 22  # every coordinate, every box extent and every product with 0.25 is then exact in float32
    return x


def ruler_positions(n, offset):
    x = ruler_x(n, offset)
    pos = np.zeros((n, 3, 3), dtype=np.float64)
    pos[:, 0, 0], pos[:, 1, 0], pos[:, 2, 0] = x, x + 0.25, x
    pos[:, 1, 1] = 0.25
    pos[:, 2, 2] = 0.25
    p32 = pos.astype(F32)
    assert np.array_equal(p32.astype(np.float64), pos)
    keys = morton_keys(p32)
    assert (np.diff(keys.astype(np.int64)) >= 0).all(), "ruler keys are not non-decreasing in x"
    assert np.array_equal(leaf_order(keys), np.arange(n)), "the ruler's leaf order is not its index order"
    return p32, x


def ruler_scene(sg, n, offset):
    """n triangles (x, 0, 0), (x + 0.25, 0.25, 0), (x, 0, 0.25) along the x axis with ruler-function gaps: the union of two runs of neighbours is
    the smaller the smaller the largest gap it spans, so agglomerative clustering by union area builds largest_gap_tree(x), whatever the radius.
    Returns (scene, x)."""
    pos, x = ruler_positions(n, offset)
    tan = np.tile(np.array([1, 0, 0], dtype=F32), (n, 3, 1))
    sc = sg.Scene(positions=pos, normals=None, texcoords=np.zeros((n, 3, 2), F32), tangents=tan, material_ids=np.zeros(n, np.uint32),
                  materials=[sg.Material(color=(0.7, 0.7, 0.7, 1.0), roughness=1.0, metallic=0.0)], textures=[],
                  camera=sg.look_camera((float(x.max()) / 2, 0.1, 3.0), yaw_deg=0.0, yfov=0.9))
    return sc, x


def triangle_boxes(positions):
    p = np.asarray(positions, dtype=F32).reshape(-1, 3, 3)
    return np.concatenate([p.min(axis=1), p.max(axis=1)], axis=1).astype(F32)


def _area(lo, hi):
    """box_area6 in float32, one rounding per operation."""
    d = (hi - lo).astype(F32)
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    a = (F32(2) * (((dx * dy).astype(F32) + (dy * dz).astype(F32)).astype(F32) + (dz * dx).astype(F32)).astype(F32)).astype(F32)
    return np.where((dx >= 0) & (dy >= 0) & (dz >= 0), a, F32(0)).astype(F32)


def ploc_replay(boxes, radius):
    """The rounds of k_ploc_nn / k_ploc_merge / k_ploc_compact over clusters that start as the (m, 6) float32 `boxes`, in order. Every cluster
    takes the neighbour within `radius` positions whose union box with it has the smallest area; ties go to the lower position, except that
    position i ^ 1 wins every tie it is part of; mutual choices merge into the lower position (left = lower); the survivors keep their order. A
    round that merges fewer than 1 / 32 of the clusters is followed by one that pairs i with i ^ 1. Returns (tree, rounds, forced rounds); the
    tree is nested (left, right) tuples over the box indices."""
    box = np.asarray(boxes, dtype=F32).copy()
    tree = list(range(len(box)))
    R = int(radius)
    rounds = forced = 0
    force = False
    while len(tree) > 1:
        m = len(tree)
        idx = np.arange(m)
        if force:
            nn = np.where((idx ^ 1) < m, idx ^ 1, idx)
            forced += 1
        else:
            best = np.full(m, np.inf, dtype=F32)
            nn = idx.copy()
            for dj in range(-R, R + 1):
                if dj == 0:
                    continue
                j = idx + dj
                ok = (j >= 0) & (j < m)
                jj = np.clip(j, 0, m - 1)
                a = _area(np.minimum(box[:, :3], box[jj, :3]), np.maximum(box[:, 3:], box[jj, 3:]))
                take = ok & ((a < best) | ((a == best) & (j == (idx ^ 1))))
                best = np.where(take, a, best)
                nn = np.where(take, j, nn)
        mutual = (nn != idx) & (nn[nn] == idx)
        new_tree, new_box = [], []
        for i in range(m):
            if not mutual[i]:
                new_tree.append(tree[i])
                new_box.append(box[i])
            elif i < nn[i]:
                j = int(nn[i])
                new_tree.append((tree[i], tree[j]))
                new_box.append(np.concatenate([np.minimum(box[i, :3], box[j, :3]), np.maximum(box[i, 3:], box[j, 3:])]))
        force = (m - len(new_tree)) * 32 < m
        tree, box = new_tree, np.array(new_box, dtype=F32)
        rounds += 1
        assert rounds <= 4096
    return tree[0], rounds, forced


# ---- a dump as a structure ---------------------------------------------------------------------------------------------------------------------
def _ref_range(ref, first, last, count):
    """Per child reference: (first record, last record, records) below it; inner references read the arrays filled so far."""
    leaf = (ref & LEAF) != 0
    b = (ref & MASK).astype(np.int64)
    c = ((ref >> 27) & 15).astype(np.int64)
    inner = np.where(leaf, 0, ref).astype(np.int64)
    return np.where(leaf, b, first[inner]), np.where(leaf, b + c - 1, last[inner]), np.where(leaf, c, count[inner])


def walk_binary(dump):
    """A bvh_device_dump walked from its root, level by level on arrays. Returns a dict of arrays indexed by inner node:
      left, right          the child references as stored;
      lfirst, llast, lcount  the lowest and highest triangle record below the left child and how many there are (rfirst, ... alike):
                             the range is contiguous where lcount == llast - lfirst + 1;
      depth                the node's depth (root 0);
    and `levels` (the inner nodes of each depth, top down), `root`, `height` (edges on the longest root-to-leaf path), `contiguous` (every child
    covers a contiguous range and the right one starts where the left one ends). Asserts that every inner record is reached exactly once and
    that every leaf reference holds 1..8 records inside the array."""
    nodes, root, n_tris = dump["nodes"], int(dump["root"]), len(dump["tris"])
    n_inner = len(nodes)
    left, right = nodes[:, 12].copy(), nodes[:, 13].copy()
    out = dict(root=root, left=left, right=right, levels=[], height=0, contiguous=True)
    z = lambda: np.full(n_inner, -1, dtype=np.int64)  # noqa: E731
    for k in ("lfirst", "llast", "lcount", "rfirst", "rlast", "rcount", "depth"):
        out[k] = z()
    if root & LEAF:
        assert n_inner == 0, "the root is a leaf but there are inner records"
        return out
    level = np.array([root], dtype=np.int64)
    seen = 0
    while len(level):
        assert (level < n_inner).all(), "a child reference names no inner record"
        assert (out["depth"][level] == -1).all() and len(np.unique(level)) == len(level), "an inner record is reached twice"
        out["depth"][level] = len(out["levels"])
        out["levels"].append(level)
        seen += len(level)
        assert seen <= n_inner
        kids = np.concatenate([left[level], right[level]])
        level = kids[(kids & LEAF) == 0].astype(np.int64)
    assert seen == n_inner, "inner nodes are not a tree over all records"
    out["height"] = len(out["levels"])
    first, last, count = z(), z(), z()
    for level in reversed(out["levels"]):
        for side, ref in (("l", left[level]), ("r", right[level])):
            leaf = (ref & LEAF) != 0
            cnt = (ref[leaf] >> 27) & 15
            assert ((cnt >= 1) & (cnt <= 8)).all() and ((ref[leaf] & MASK).astype(np.int64) + cnt <= n_tris).all(), "a leaf reference leaves the records"
            f, l, c = _ref_range(ref, first, last, count)
            out[side + "first"][level], out[side + "last"][level], out[side + "count"][level] = f, l, c
        first[level] = np.minimum(out["lfirst"][level], out["rfirst"][level])
        last[level] = np.maximum(out["llast"][level], out["rlast"][level])
        count[level] = out["lcount"][level] + out["rcount"][level]
    assert count[root] == n_tris and first[root] == 0 and last[root] == n_tris - 1, "the leaves do not cover the triangle records"
    out["contiguous"] = bool((out["lcount"] == out["llast"] - out["lfirst"] + 1).all() and (out["rcount"] == out["rlast"] - out["rfirst"] + 1).all()
                             and (out["rfirst"] == out["llast"] + 1).all())
    return out


def nested(dump):
    """The tree of a dump as nested (left, right) tuples, whatever its records are numbered. A leaf of one record is its record index, a leaf of
    several the range of them. For small trees (recursive)."""
    nodes = dump["nodes"]

    def build(ref, depth):
        assert depth <= 64
        if ref & LEAF:
            b, c = ref & MASK, (ref >> 27) & 15
            return b if c == 1 else range(b, b + c)
        return (build(int(nodes[ref, 12]), depth + 1), build(int(nodes[ref, 13]), depth + 1))

    return build(int(dump["root"]), 0)


def child_boxes(dump, walk, positions):
    """(n_inner, 12) float32: the exact boxes {left lo, left hi, right lo, right hi} of every inner node's children, bottom up and level by level
    from the vertices of the triangles the records name (word 9)."""
    nodes, tris = dump["nodes"], dump["tris"]
    v = np.asarray(positions, dtype=F32).reshape(-1, 3, 3)[tris[:, 9]]
    tlo, thi = v.min(axis=1), v.max(axis=1)
    n_inner = len(nodes)
    want = np.zeros((n_inner, 12), dtype=F32)
    nlo, nhi = np.zeros((n_inner, 3), dtype=F32), np.zeros((n_inner, 3), dtype=F32)
    for level in reversed(walk["levels"]):
        for k, ref in ((0, nodes[level, 12]), (6, nodes[level, 13])):
            leaf = (ref & LEAF) != 0
            b = np.where(leaf, ref & MASK, 0).astype(np.int64)
            c = np.where(leaf, (ref >> 27) & 15, 1).astype(np.int64)
            lo, hi = tlo[b].copy(), thi[b].copy()
            for t in range(1, 8):  # a leaf holds at most 8 records
                more = c > t
                if not more.any():
                    break
                lo[more] = np.minimum(lo[more], tlo[b[more] + t])
                hi[more] = np.maximum(hi[more], thi[b[more] + t])
            inner = np.where(leaf, 0, ref).astype(np.int64)
            lo = np.where(leaf[:, None], lo, nlo[inner])
            hi = np.where(leaf[:, None], hi, nhi[inner])
            want[level, k : k + 3], want[level, k + 3 : k + 6] = lo, hi
        nlo[level] = np.minimum(want[level, 0:3], want[level, 6:9])
        nhi[level] = np.maximum(want[level, 3:6], want[level, 9:12])
    return want
