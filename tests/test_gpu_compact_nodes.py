"""wf_extend's two-visit node step (csrc/rt_dev_trav.h trav_step_inner_fast) and the compact records it reads, on the GPU against the oracle.

A lane that steps straight into an inner child visits it in the same trip from the child's 32-byte compact record. The lanes visit the same
nodes in the same order as before, two to a trip, so hits, framebuffers and every event counter must stay the oracle's bit for bit: on the
600-triangle golden scenes and a 4 096-triangle room, through rt_cast_rays_ex and a 64x48x4 render with counters; on a tree deeper than the
LDS ring of wf_extend's stack (second visits push frames past ring depth); on queues shorter than a wave (only the sparse drain runs); after
rt_update_geometry; and on a tree patched to be looser than its builder left it, where the affected child must lose `valid`.
(RT_UPDATE_REFIT refits the 8-wide tree only; a binary scene refuses it, so the update case is REBUILD.)
The records in HBM are what rt_compact_derive_host (the same function, tests/test_compact_nodes.py) makes of the dumped nodes."""
import numpy as np
import pytest

import deep_walks as dw
from conftest import golden_scene_specs, make_scene, random_rays
from test_compact_nodes import VALID, check_tree, room4096

pytestmark = pytest.mark.gpu

LEAF = 0x80000000
COUNTERS = ("samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests",
            "light_tri_tests", "light_hits", "texel_fetches")
SCENES = list(golden_scene_specs()) + ["room4096"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def scene_of(sg, name):
    return room4096(sg) if name == "room4096" else make_scene(sg, golden_scene_specs()[name])


def assert_records_are_the_host_derivation(gpu, dev):
    """The sel words and compact records in HBM equal the host run of the same rule on the dumped nodes, and every valid child expands."""
    nodes, compact = dev.bvh_device_dump(0)["nodes"], dev.bvh_compact_dump()
    derived, want, n_valid = check_tree(gpu, nodes)
    assert np.array_equal(nodes[:, 14], derived[:, 14]) and np.array_equal(compact, want)
    return nodes, n_valid


def assert_hits_are_the_oracles(gpu, dev, orc, rays, what):
    """rt_cast_rays_ex through wf_extend in the reference's traversal order (global-best pruning on this tree: tests/test_gpu_production.py)."""
    op, ob = orc.cast_rays(rays)
    gp, gb, st = dev.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
    assert np.array_equal(gp, op) and np.array_equal(bits(gb), bits(ob)), f"{what}: {int((gp != op).sum())} of {len(rays)} hits differ from the oracle"
    return st


@pytest.mark.parametrize("name", SCENES)
def test_casts_and_render_are_the_oracles(gpu, oracle, sg, name):
    sc = scene_of(sg, name)
    dev, orc = gpu.DeviceScene(sc), oracle.OracleScene(sc)
    try:
        nodes, n_valid = assert_records_are_the_host_derivation(gpu, dev)
        assert n_valid == len(nodes) - 1, "a host-built tree: every inner child but the root has a compact record"
        assert_hits_are_the_oracles(gpu, dev, orc, random_rays(sc, 6000, seed=3), name)
        assert dev.second_visits() > 0, "no node was visited from its compact record"
        W, H, SPP = 64, 48, 4
        ofb, ost = orc.run_raytracer(W, H, SPP, seed=9)
        gfb, gst = dev.run_raytracer(W, H, SPP, seed=9, counters=True)
        share = dev.second_visits() / gst["nodes_visited"]
        print(f"[compact nodes] {name}: {dev.second_visits()} of {gst['nodes_visited']} node visits ({share:.1%}) from a compact record")
        assert np.array_equal(bits(gfb), bits(ofb)), f"{int((bits(gfb) != bits(ofb)).any(axis=2).sum())} pixels differ from the oracle"
        for k in COUNTERS:
            assert gst[k] == ost[k], f"counter {k}: gpu {gst[k]} oracle {ost[k]}"
        assert dev.second_visits() > 0
        nfb, _ = dev.run_raytracer(W, H, SPP, seed=9)  # the instantiation without counters
        assert np.array_equal(bits(nfb), bits(ofb))
    finally:
        dev.close()
        orc.close()


@pytest.mark.parametrize("builder", ["ploc", "lbvh"])
def test_device_built_trees_get_their_records(gpu, oracle, sg, builder):
    """Both device builders leave their DevNode array in HBM; the records are derived there. Closest-hit distances are the oracle's."""
    sc = room4096(sg)
    kw = {"device_builder": gpu.RT_BUILDER_LBVH} if builder == "lbvh" else {}
    dev, orc = gpu.DeviceScene(sc, device_bvh=True, **kw), oracle.OracleScene(sc)
    try:
        nodes, n_valid = assert_records_are_the_host_derivation(gpu, dev)
        print(f"[compact nodes] {builder}: {n_valid} of {len(nodes) - 1} inner children valid")
        assert n_valid == len(nodes) - 1, "the builders' refit makes every box the exact union of its children's"
        rays = random_rays(sc, 6000, seed=4)
        _, ob = orc.cast_rays(rays)
        _, gb, _ = dev.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
        assert np.array_equal(bits(gb[:, 2]), bits(ob[:, 2]))
        assert dev.second_visits() > 0
    finally:
        dev.close()
        orc.close()


def test_rebuild_derives_the_records_again(gpu, oracle, sg):
    sc, sc2 = room4096(sg), sg.room_scene(4096, seed=6, n_lights=4, n_materials=6, tex_size=0)
    dev, orc2 = gpu.DeviceScene(sc), oracle.OracleScene(sc2)
    try:
        before = dev.bvh_compact_dump()
        dev.update_geometry(sc2)
        nodes, n_valid = assert_records_are_the_host_derivation(gpu, dev)
        assert n_valid == len(nodes) - 1 and not np.array_equal(before, dev.bvh_compact_dump())
        assert_hits_are_the_oracles(gpu, dev, orc2, random_rays(sc2, 6000, seed=5), "after REBUILD")
        with pytest.raises(gpu.RtError):  # a binary tree is never refitted: there is no second way for its records to go stale
            dev.update_geometry(sc, refit=True)
    finally:
        dev.close()
        orc2.close()


def test_a_looser_tree_loses_valid_and_keeps_its_hits(gpu, oracle, sg):
    """Boxes moved outwards in HBM (rt_bvh_patch_plane): a correct tree, looser than its children's union at those nodes. The children of the
    looser boxes lose `valid` and are visited from their DevNode; the hits stay the oracle's."""
    sc = room4096(sg)
    dev, orc = gpu.DeviceScene(sc), oracle.OracleScene(sc)
    try:
        nodes, n_base = assert_records_are_the_host_derivation(gpu, dev)
        rays = random_rays(sc, 6000, seed=6)
        picked = [(i, s) for i in range(len(nodes)) for s in (0, 1) if not nodes[i, 12 + s] & LEAF][:: max(1, len(nodes) // 40)]
        for n, (i, side) in enumerate(picked):
            f = n % 6
            v = float(nodes[i, 6 * side + f : 6 * side + f + 1].view(np.float32)[0])
            dev.bvh_patch_plane(i, 6 * side + f, v - 0.25 if f < 3 else v + 0.25)
        after, n_valid = assert_records_are_the_host_derivation(gpu, dev)
        for i, side in picked:
            assert ((int(after[i, 14]) >> (8 * side)) & VALID) == 0, f"node {i} side {side}: the child of a looser box kept valid"
        assert n_valid < n_base
        op, ob = orc.cast_rays(rays)
        gp, gb, _ = dev.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
        assert np.array_equal(gp, op) and np.array_equal(bits(gb), bits(ob))
        assert dev.second_visits() > 0
        ofb, _ = orc.run_raytracer(64, 48, 2, seed=11)
        nfb, _ = dev.run_raytracer(64, 48, 2, seed=11)  # the instantiation without counters, on the mixed tree
        assert np.array_equal(bits(nfb), bits(ofb))
    finally:
        dev.close()
        orc.close()


def test_second_visits_push_frames_past_the_lds_ring(gpu, oracle, sg):
    """20 000 needles: the SAH tree's boxes overlap at every level. The oracle's census of the test's own rays shows that enough of them
    hold 8 or more deferred siblings (the first eviction of wf_extend's 6-deep ring); a second visit that pushes there spills like a first."""
    sc = dw.needle_soup_scene(sg, **dw.NEEDLES)
    dev, orc = gpu.DeviceScene(sc), oracle.OracleScene(sc)
    try:
        rays = dw.light_query_rays(sc, 4000, 79)
        closest, _ = orc.walk_census(rays)
        dw.require_witnesses("needles, two-visit casts", closest, {dw.CLOSEST_RING_EVICT: 0.01})
        assert_hits_are_the_oracles(gpu, dev, orc, rays, "needles")
        assert dev.second_visits() > 0
        W, H, SPP = 48, 40, 2
        ofb, ost = orc.run_raytracer(W, H, SPP, seed=23)
        gfb, gst = dev.run_raytracer(W, H, SPP, seed=23, counters=True)
        assert np.array_equal(bits(gfb), bits(ofb))
        for k in COUNTERS:
            assert gst[k] == ost[k], k
        nfb, _ = dev.run_raytracer(W, H, SPP, seed=23)  # wf_extend<false, false>: the instantiation the register barrier is for
        assert np.array_equal(bits(nfb), bits(ofb))
    finally:
        dev.close()
        orc.close()


@pytest.mark.parametrize("n_rays", [1, 20, 32, 63])
def test_queues_shorter_than_a_wave(gpu, oracle, sg, n_rays):
    """A queue of fewer than 64 rays is used up by the one wave's first ticket; at 32 rays or fewer that wave leaves its loop after the first
    leaf batch and the sparse drain, which calls the same node step, walks the rest."""
    sc = room4096(sg)
    dev, orc = gpu.DeviceScene(sc), oracle.OracleScene(sc)
    try:
        assert_hits_are_the_oracles(gpu, dev, orc, random_rays(sc, n_rays, seed=7), f"{n_rays} rays")  # some axis-parallel: see below
        # random_rays puts its axis-parallel rays first (64 of 1024). Such a ray is outside the exact-quotient division's range, and a wave
        # takes the general step, which makes no second visit, for as long as one of its lanes walks one: so the claim is made of rays
        # that all have the guarantee.
        assert_hits_are_the_oracles(gpu, dev, orc, random_rays(sc, 1024, seed=7)[64 : 64 + n_rays], f"{n_rays} fast rays")
        # (one counter for the whole walk: it cannot tell the drain's second visits from those of the trips before the first leaf batch;
        # what pins the drain is that hits and every counter of walks that end in it are the oracle's)
        assert dev.second_visits() > 0, "a walk through the loop and the sparse drain made no second visit"
        W, H, SPP = 5, 4, 1  # 20 primary rays, fewer at every later bounce
        ofb, ost = orc.run_raytracer(W, H, SPP, seed=3)
        gfb, gst = dev.run_raytracer(W, H, SPP, seed=3, counters=True)
        assert np.array_equal(bits(gfb), bits(ofb))
        for k in COUNTERS:
            assert gst[k] == ost[k], k
        nfb, _ = dev.run_raytracer(W, H, SPP, seed=3)  # without counters
        assert np.array_equal(bits(nfb), bits(ofb))
    finally:
        dev.close()
        orc.close()
