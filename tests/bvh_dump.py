"""The binary BVH as it sits in HBM (DeviceScene.bvh_device_dump: DevNode / DevTri records, DESIGN.md 'Data layout in HBM'), restated in numpy.

A plain module next to the tests. `flatten_reference` turns a reference-style node list (bvh_info) into those records: tests/test_gpu_bvh_device.py
compares it with what a host-built scene holds in HBM, tests/test_walk_census.py feeds it to deep_walks.dump_census.

A child reference (words 12 and 13 of a node record, and the root) is an inner-node index, or LEAF | count << 27 | first triangle record for a
leaf of 1..8 triangles (count 0: the leaf ends at the record whose flag word, word 10, has bit 0 set)."""
import numpy as np

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
