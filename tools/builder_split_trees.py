#!/usr/bin/env python3
"""tools/builder_split_trees.py [--tree DIR] — one digest line per device build of the small scenes of tests/test_gpu_device_builders.py, for
comparing the trees of two built checkouts bit for bit (profiles/builder_split_trees.txt: the parent commit against the split of
rt_bvh_device.hip). --tree DIR loads the library of another built checkout; scenes and readers are this checkout's in both runs.

Per scene: the binary tree with device_builder = PLOC and = LBVH and lbvh_leaf_tris = 1 and 3 (rt_bvh_device_dump), and the wide tree of both
builders (rt_bvh_wide_dump). The radix builder's dump is hashed word for word. PLOC numbers its inner nodes by an atomic and the collapse its
records and triangle runs by atomics, so those are hashed as structures, in depth-first order from the root: a binary node is its sixteen
words with child indices replaced by the subtree that follows; a wide node is its origin and exponent bits, masks, all 48 plane bytes, then
its inner children in slot order and the whole triangle records of its leaf slots (every word but DevTri::pad)."""
import argparse, hashlib, importlib, os, sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=None, help="another built checkout whose library is loaded")
args = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, os.path.abspath(args.tree) if args.tree else HERE)
import numpy as np
import torch  # noqa: F401  (before the library: bench.py's rule)

rt = importlib.import_module("raytracing-course-hw-public_amd")
import lbvh_replay as lr
import test_gpu_device_builders as tb

LEAF, MASK = 0x80000000, 0x07FFFFFF
sg = rt.scenegen
rt.lib()


def binary_digest(dump, structural):
    h = hashlib.sha256()
    h.update(dump["tris"].tobytes())
    nodes = dump["nodes"]
    if not structural:
        h.update(np.uint32(dump["root"]).tobytes() + nodes.tobytes())
        return h.hexdigest()[:16], 0
    stack, seen = [int(dump["root"])], 0
    while stack:
        ref = stack.pop()
        if ref & LEAF:
            h.update(b"L" + np.uint32(ref).tobytes())
            continue
        seen += 1
        row = nodes[ref]
        h.update(b"N" + row[0:12].tobytes() + row[14:16].tobytes())
        stack += [int(row[13]), int(row[12])]  # left first
    assert seen == len(nodes)
    return h.hexdigest()[:16], seen


def wide_digest(dump):
    nodes, tris = dump["nodes"], dump["tris"]
    b = nodes.view(np.uint8).reshape(len(nodes), 80)
    h = hashlib.sha256()
    h.update(np.uint32(dump["depth"]).tobytes())
    stack, seen, seen_tris = [0], 0, 0
    while stack:
        i = stack.pop()
        seen += 1
        h.update(b[i, 0:16].tobytes() + nodes[i, 6:8].tobytes() + b[i, 32:80].tobytes())  # origin, exponents, imask; tri_mask, pad; planes
        n_inner, n_tri = bin(int(b[i, 15])).count("1"), bin(int(nodes[i, 6])).count("1")
        base, tb0 = int(nodes[i, 4]), int(nodes[i, 5])
        stack += [base + r for r in reversed(range(n_inner))]  # slot order
        h.update(tris[tb0 : tb0 + n_tri, 0:11].tobytes())  # leaf slots' triangles, slot by slot
        seen_tris += n_tri
    assert seen == len(nodes) and seen_tris == len(tris)
    return h.hexdigest()[:16], seen


scenes = [(n, tb._scene(sg, n)) for n in ("room_5000", "planar", "soup_9", "one_cell")]
scenes += [(f"ruler_{n}", lr.ruler_scene(sg, n, off)[0]) for n, off in ((257, 255), (513, 3))]
for name, sc in scenes:
    for builder in ("ploc", "lbvh"):
        opts = {"device_builder": rt.RT_BUILDER_LBVH} if builder == "lbvh" else {}
        for leaf_tris in (1, 3):
            dev = rt.DeviceScene(sc, device_bvh=True, lbvh_leaf_tris=leaf_tris, **opts)
            try:
                d, n = binary_digest(dev.bvh_device_dump(0), structural=builder == "ploc")
            finally:
                dev.close()
            print(f"{name:10s} {builder} leaf_tris={leaf_tris} binary {'structure' if builder == 'ploc' else 'words    '} {d}  inner nodes {n if builder == 'ploc' else '-'}", flush=True)
        dev = rt.DeviceScene(sc, device_bvh=True, wide=True, **opts)
        try:
            d, n = wide_digest(dev.bvh_wide_dump())
        finally:
            dev.close()
        print(f"{name:10s} {builder} wide               structure {d}  wide nodes {n}", flush=True)
