"""GPU tests of wf_extend's sparse drain (csrc/rt_wf_extend.hip): once a wave's queue is used up and at most RT_EXT_SPARSE_MAX of its lanes
still walk, it leaves the throughput loop for one that unwinds fully, tests waiting leaves at once and steps inner nodes in the same trip.
Every lane runs the same state machine in the same order, so hits and counters must not change.

A launch of a few rays is sparse from its first trips: with 1 or 5 rays the only wave that gets work finds the queue used up at its first
refill; 63 and 65 rays put a full and a nearly empty wave side by side; 300 rays are five waves that go sparse one after the other. A small
render's later bounces are such launches too."""
import numpy as np
import pytest

import deep_walks as dw
from conftest import random_rays
from guarded_rays import big_leaf_scene

pytestmark = pytest.mark.gpu

COUNTS = (1, 5, 63, 65, 300)
COUNTERS = ("samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests",
            "light_tri_tests", "light_hits", "texel_fetches")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cases(gpu, oracle, sg, scenes):
    """name -> (device scene, 300 rays, the oracle's hits of them), made once; nobody writes to the arrays."""
    made = {
        "room_textured": scenes["room_textured"],        # a small golden scene
        "big_leaves": big_leaf_scene(sg),                # leaves beyond 8 triangles: the triangle-by-triangle walker
        "needles": dw.needle_soup_scene(sg, **dw.NEEDLES),  # stacks beyond the LDS tier of wf_extend's ring
    }
    out = {}
    for name, sc in made.items():
        rays = dw.light_query_rays(sc, 300, 79) if name == "needles" else random_rays(sc, 300, seed=23)
        orc = oracle.OracleScene(sc)
        op, ob = orc.cast_rays(rays)
        closest, _ = orc.walk_census(rays)
        orc.close()
        for a in (rays, op, ob):
            a.setflags(write=False)
        out[name] = (gpu.DeviceScene(sc), rays, op, ob, closest)
    yield out
    for dev, *_ in out.values():
        dev.close()


def test_the_fixtures_reach_what_they_claim(cases):
    dev, rays, op, _, _ = cases["big_leaves"]
    info = dev.bvh_info(0)
    assert (info["nodes"][:, 9] - info["nodes"][:, 8])[info["nodes"][:, 6] == 0xFFFFFFFF].max() > 8
    for name, (_, _, op, _, closest) in cases.items():
        assert (op != 0xFFFFFFFF).sum() >= 30, name
    _, _, _, _, closest = cases["needles"]
    for n in COUNTS[2:]:  # walks whose 8th pending frame evicts the ring's oldest
        assert (np.asarray(closest[:n]) >= dw.CLOSEST_RING_EVICT).mean() >= 0.25, n


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", ["room_textured", "big_leaves", "needles"])
def test_few_rays_through_wf_extend(gpu, cases, name, n):
    dev, rays, op, ob, _ = cases[name]
    r = rays[:n]
    gp, gb, st = dev.cast_rays_ex(r, gpu.RT_CAST_EXTEND)
    assert np.array_equal(gp, op[:n]), (name, n, np.nonzero(gp != op[:n])[0][:8])
    assert np.array_equal(bits(gb), bits(ob[:n])), (name, n)
    # parity mode: the visits are the reference's, which the packet kernel (no refill, no leaf batches, no drain) counts too
    _, _, packet = dev.cast_rays_ex(r, gpu.RT_CAST_PACKET)
    assert st["casts"] == n
    for k in ("casts", "nodes_visited", "box_tests", "tri_tests"):
        assert st[k] == packet[k], (name, n, k, st[k], packet[k])
    assert st["nodes_visited"] > 0
    gp, gb, gst = dev.cast_rays_ex(r, gpu.RT_CAST_EXTEND_GLOBAL)
    assert np.array_equal(gp, op[:n]), (name, n, "global best", np.nonzero(gp != op[:n])[0][:8])
    assert np.array_equal(bits(gb), bits(ob[:n])), (name, n, "global best")
    assert 0 < gst["nodes_visited"] <= st["nodes_visited"]


@pytest.mark.parametrize("sort", ["sort_off", "sort_octant_cell_cone"])
@pytest.mark.parametrize("name", ["room_textured", "boxes"])
def test_short_queues_of_awkward_length(gpu, oracle, scenes, name, sort):
    """24 x 20 at 3 samples: 1440 primary rays and fewer at every later bounce, far below the resident lane count and no multiple of 64, so
    every wave of every bounce that gets rays at all ends in the sparse drain. The oracle's image and counters."""
    W, H, SPP = 24, 20, 3
    sc = scenes[name]
    dev, orc = gpu.DeviceScene(sc), oracle.OracleScene(sc)
    try:
        ofb, ost = orc.run_raytracer(W, H, SPP, seed=5)
        mode = gpu.RT_SORT_OFF if sort == "sort_off" else gpu.RT_SORT_OCTANT_CELL_CONE
        for pkt in (gpu.RT_PACKET_OFF, gpu.RT_PACKET_ON):
            gfb, gst = dev.run_raytracer(W, H, SPP, seed=5, counters=True, sort_mode=mode, packet_mode=pkt)
            assert np.array_equal(bits(gfb), bits(ofb)), (name, sort, pkt, int((bits(gfb) != bits(ofb)).any(axis=2).sum()))
            for k in COUNTERS:
                assert gst[k] == ost[k], (name, sort, pkt, k, gst[k], ost[k])
        plain, _ = dev.run_raytracer(W, H, SPP, seed=5, sort_mode=mode, packet_mode=gpu.RT_PACKET_OFF)  # the kernels without counters
        assert np.array_equal(bits(plain), bits(ofb))
        assert ost["casts"] > W * H * SPP and (W * H * SPP) % 64 != 0
    finally:
        dev.close()
        orc.close()
