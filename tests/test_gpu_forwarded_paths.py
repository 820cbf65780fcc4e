"""GPU tests of the sorted bounces' queue handling (csrc/rt_wavefront.hip, csrc/rt_wf_shade.hip, csrc/rt_wf_policy.h, csrc/rt_ray_key.h): a bounce that may be followed by a sorted one has
wf_shade write the ray-order sort's input itself, key and slot at the physical slot of every ray it makes (WfLaunch::emit_keys), and the sort
runs over the queue's physical positions: the filled parts of the 64 sub-queue regions and, between them, the unfilled ends, which hold pad
keys. A pad that does not lose against a real key, a slot left without its key, or a sort that is too short loses or duplicates a ray, which
shows as differing pixels or as a `samples` / `casts` mismatch. (The file keeps the name of the first half of the work it was written for:
forwarding the path records to their queue positions was built, measured slower and left out, profiles/forwarded_paths.txt.)

The automatic mode sorts nothing below 2^20 paths, so every render here forces RT_SORT_OCTANT_CELL_CONE; a bounce is sorted only while the
host's bound of its queue is >= 4096 rays. 96 x 96 at 2 samples are 18 432 paths = 288 wave slots over 64 sub-queue regions: no region of
any bounce is full, so every sorted queue has gaps between its regions.

What is compared: the parity build against the oracle (image bits and all twelve event counters) and against its own RT_SORT_OFF render.
The production traversals (RT_FLAG_GLOBAL_BEST on the binary tree; the wide tree, host and device built) may differ from the oracle on exact
ties by contract (tests/test_gpu_production.py explains those pixels), so they are held to what this change can move: the forced
sort render equals, bit for bit, the RT_SORT_OFF render of the same scene object, which sorts nothing, with the same counters."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 96, 96, 2, 31
COUNTERS = ("samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests",
            "light_tri_tests", "light_hits", "texel_fetches")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scene(scenes):
    sc = dataclasses.replace(scenes["room_textured"], ray_depth=8)
    return sc


@pytest.fixture(scope="module")
def ref(oracle, scene):
    """The oracle's image and counters of the one render every test here repeats, made once; nobody writes to the image."""
    orc = oracle.OracleScene(scene)
    fb, st = orc.run_raytracer(W, H, SPP, seed=SEED)
    orc.close()
    fb.setflags(write=False)
    return fb, st


def test_parity_build_against_the_oracle(gpu, scene, ref):
    ofb, ost = ref
    assert W * H * SPP >= 4096 and ost["casts"] > 2 * W * H * SPP  # bounce 1 is sorted, and paths go on behind it
    dev = gpu.DeviceScene(scene)
    try:
        for pkt in (gpu.RT_PACKET_OFF, gpu.RT_PACKET_ON):
            gfb, gst = dev.run_raytracer(W, H, SPP, seed=SEED, counters=True, sort_mode=gpu.RT_SORT_OCTANT_CELL_CONE, packet_mode=pkt)
            assert np.array_equal(bits(gfb), bits(ofb)), (pkt, int((bits(gfb) != bits(ofb)).any(axis=2).sum()))
            for k in COUNTERS:
                assert gst[k] == ost[k], (pkt, k, gst[k], ost[k])
        plain, _ = dev.run_raytracer(W, H, SPP, seed=SEED, sort_mode=gpu.RT_SORT_OCTANT_CELL_CONE)  # the kernels without counters
        assert np.array_equal(bits(plain), bits(ofb)), int((bits(plain) != bits(ofb)).any(axis=2).sum())
        off, _ = dev.run_raytracer(W, H, SPP, seed=SEED, sort_mode=gpu.RT_SORT_OFF)
        assert np.array_equal(bits(plain), bits(off))
    finally:
        dev.close()


@pytest.mark.parametrize("build", ["global_best", "wide_host", "wide_device"])
def test_production_builds_against_their_unsorted_render(gpu, scene, ref, build):
    _, ost = ref
    kw = {"global_best": {}, "wide_host": dict(wide=True), "wide_device": dict(wide=True, device_bvh=True)}[build]
    rkw = dict(global_best=True) if build == "global_best" else {}
    dev = gpu.DeviceScene(scene, **kw)
    try:
        on, son = dev.run_raytracer(W, H, SPP, seed=SEED, counters=True, sort_mode=gpu.RT_SORT_OCTANT_CELL_CONE, **rkw)
        off, soff = dev.run_raytracer(W, H, SPP, seed=SEED, counters=True, sort_mode=gpu.RT_SORT_OFF, **rkw)
        assert np.array_equal(bits(on), bits(off)), (build, int((bits(on) != bits(off)).any(axis=2).sum()))
        for k in COUNTERS:  # the order of the rays changes no path and no walk
            assert son[k] == soff[k], (build, k, son[k], soff[k])
        assert son["samples"] == ost["samples"] == W * H * SPP
        plain, _ = dev.run_raytracer(W, H, SPP, seed=SEED, sort_mode=gpu.RT_SORT_OCTANT_CELL_CONE, **rkw)
        assert np.array_equal(bits(plain), bits(off)), build
    finally:
        dev.close()


def test_last_sorted_bounce_below_one_wave_slot_per_region(gpu, oracle, scenes):
    """66 x 64 at 1 sample: 4224 primary rays, so bounce 1 is sorted (the host's bound is the pass size), but fewer than 64 x 64 = 4096 of
    them survive bounce 0 in the open room (checked below from the oracle: with ray_depth 2, casts = primary rays + survivors of bounce 0).
    Bounce 1's queue then has regions that hold less than one wave slot, some possibly nothing, and no later bounce is sorted."""
    w, h = 66, 64
    sc = dataclasses.replace(scenes["open_nolight"], ray_depth=8)
    orc2 = oracle.OracleScene(dataclasses.replace(sc, ray_depth=2))
    _, st2 = orc2.run_raytracer(w, h, 1, seed=SEED)
    orc2.close()
    assert w * h >= 4096 and 0 < st2["casts"] - w * h < 4096
    orc, dev = oracle.OracleScene(sc), gpu.DeviceScene(sc)
    try:
        ofb, ost = orc.run_raytracer(w, h, 1, seed=SEED)
        gfb, gst = dev.run_raytracer(w, h, 1, seed=SEED, counters=True, sort_mode=gpu.RT_SORT_OCTANT_CELL_CONE)
        assert np.array_equal(bits(gfb), bits(ofb)), int((bits(gfb) != bits(ofb)).any(axis=2).sum())
        for k in COUNTERS:
            assert gst[k] == ost[k], (k, gst[k], ost[k])
        plain, _ = dev.run_raytracer(w, h, 1, seed=SEED, sort_mode=gpu.RT_SORT_OCTANT_CELL_CONE)
        assert np.array_equal(bits(plain), bits(ofb))
    finally:
        dev.close()
        orc.close()


def test_three_shards_end_mid_region(gpu, scene, ref):
    """shard_count = 3 with blocks of 64 pixels: each shard renders 48 of the 144 blocks = 6144 paths per pass (sorted at bounce 1), whose
    queues end in the middle of a region. The union of the shards is the oracle's image; their counters add up to the oracle's."""
    ofb, ost = ref
    dev = gpu.DeviceScene(scene)
    try:
        sh = np.zeros_like(ofb)
        total = dict.fromkeys(COUNTERS, 0)
        for r in range(3):
            _, st = dev.run_raytracer(W, H, SPP, seed=SEED, counters=True, shard_index=r, shard_count=3, shard_block=64, out=sh,
                                      sort_mode=gpu.RT_SORT_OCTANT_CELL_CONE)
            for k in COUNTERS:
                total[k] += st[k]
        assert np.array_equal(bits(sh), bits(ofb)), int((bits(sh) != bits(ofb)).any(axis=2).sum())
        for k in COUNTERS:
            assert total[k] == ost[k], (k, total[k], ost[k])
    finally:
        dev.close()
