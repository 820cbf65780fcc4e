"""GPU tests of the camera-relative records of the primary-ray packet kernel (csrc/rt_wf_extend.hip: wf_camera_relative, wf_extend_packet<.., REL>).

A pass of camera rays of ONE view walks a copy of the binary tree's records with the camera position folded in; every other pass (several
views, caller-supplied rays, packets off) walks the tree's own records. Nothing a caller sees may tell the two apart: framebuffers are compared
bit for bit and event counters exactly, against the per-lane kernel (packets off) and against the CPU oracle. The copy is kept per (camera
position, tree), so the tests also change the camera and the geometry under a live scene and compare with fresh scenes.

Every render here is 40 x 36 at 16 samples unless a test says otherwise: 23 040 paths, for which the copy of each of these scenes is made
(csrc/rt_render.cpp camera_relative_records: at most 16 bytes of records per path of the pass)."""
import dataclasses

import numpy as np
import pytest

from conftest import random_rays
from guarded_rays import big_leaf_scene
from update_geometry import deform, relight

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 40, 36, 16, 77
FIXTURES = ["room_plain", "room_textured", "open_nolight", "boxes", "room_manylights"]
COUNTERS = ("samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests",
            "light_tri_tests", "light_hits", "texel_fetches")
REL_BYTES_PER_PATH = 16  # RT_REL_BYTES_PER_PATH of csrc/rt_render.cpp


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def copy_is_made(dev, n_paths):
    """The size rule of camera_relative_records, from the tree's own counts: a test that means to exercise the copy asserts this first."""
    info = dev.bvh_info(0)
    nodes = info["nodes"]
    n_inner = int((nodes[:, 6] != 0xFFFFFFFF).sum())
    n_tris = len(info["order"])
    return n_inner > 0 and 64 * n_inner + 48 * n_tris <= REL_BYTES_PER_PATH * n_paths


def on_off_oracle(gpu, oracle, sc, w=W, h=H, spp=SPP, seed=SEED):
    """Packets on (camera-relative records), packets off (wf_extend) and the oracle: one image, one set of counters. Returns the image."""
    dev, orc = gpu.DeviceScene(sc), oracle.OracleScene(sc)
    try:
        assert copy_is_made(dev, w * h * spp)
        ofb, ost = orc.run_raytracer(w, h, spp, seed=seed)
        on, on_st = dev.run_raytracer(w, h, spp, seed=seed, counters=True, packet_mode=gpu.RT_PACKET_ON)
        off, off_st = dev.run_raytracer(w, h, spp, seed=seed, counters=True, packet_mode=gpu.RT_PACKET_OFF)
        assert on_st["packet_passes"] == on_st["passes"] == 1 and off_st["packet_passes"] == 0
        assert np.array_equal(bits(on), bits(off)), f"{int((bits(on) != bits(off)).any(axis=2).sum())} pixels differ between packets on and off"
        assert np.array_equal(bits(on), bits(ofb)), f"{int((bits(on) != bits(ofb)).any(axis=2).sum())} pixels differ from the oracle"
        for k in COUNTERS:
            assert on_st[k] == off_st[k] == ost[k], (k, on_st[k], off_st[k], ost[k])
        plain, _ = dev.run_raytracer(w, h, spp, seed=seed, packet_mode=gpu.RT_PACKET_ON)  # the kernel without counters is another instantiation
        assert np.array_equal(bits(plain), bits(ofb))
        gb_on, _ = dev.run_raytracer(w, h, spp, seed=seed, packet_mode=gpu.RT_PACKET_ON, global_best=True)  # ... and so are the global-best ones
        gb_off, _ = dev.run_raytracer(w, h, spp, seed=seed, packet_mode=gpu.RT_PACKET_OFF, global_best=True)
        assert np.array_equal(bits(gb_on), bits(gb_off))
        return on
    finally:
        dev.close()
        orc.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_packets_on_equal_packets_off_and_the_oracle(gpu, oracle, scenes, name):
    fb = on_off_oracle(gpu, oracle, scenes[name])
    assert np.isfinite(fb).all() and np.count_nonzero(fb) > 0


@pytest.mark.parametrize("case", ["zero_component", "tiny_component", "both"])
def test_cameras_outside_the_fast_division_range(gpu, oracle, sg, case):
    """A camera position with a component of 0 keeps the exact-quotient shortcut (corner - 0 is the corner); one with a component of magnitude
    below 2^-37 sends every primary ray through the reference's IEEE division. Both read the folded corners."""
    sc = sg.room_scene(300, seed=41, n_lights=3, n_materials=5, tex_size=8, n_tex_sets=2)
    pos = np.asarray(sc.camera.position, dtype=np.float32).copy()
    if case in ("zero_component", "both"):
        pos[1] = np.float32(0.0)
    if case in ("tiny_component", "both"):
        pos[2] = np.float32(-1e-13)
    assert abs(float(np.float32(-1e-13))) < 2.0**-37
    sc.camera.position = pos
    on_off_oracle(gpu, oracle, sc)


def test_big_leaves_and_duplicate_geometry(gpu, oracle, sg):
    """Leaves beyond 8 triangles are walked with the per-triangle flags, which the folded records keep; duplicate triangles tie in t, and the
    first in leaf order must win whichever records are read."""
    sc = big_leaf_scene(sg)
    dev = gpu.DeviceScene(sc)
    info = dev.bvh_info(0)
    leaf_sizes = (info["nodes"][:, 9] - info["nodes"][:, 8])[info["nodes"][:, 6] == 0xFFFFFFFF]
    dev.close()
    assert leaf_sizes.max() > 8
    on_off_oracle(gpu, oracle, sc)


def test_a_new_camera_gets_a_new_copy(gpu, sg, scenes):
    """Two cameras one after the other on one scene, then the first again: each render is the render of a fresh scene with that camera."""
    sc = scenes["room_textured"]
    p = np.asarray(sc.camera.position, dtype=np.float32)
    cams = [sc.camera, sg.look_camera(p + np.float32(0.75), yaw_deg=25.0, yfov=0.7, aspect=W / H), sg.look_camera(p * np.float32(0.5), yaw_deg=-40.0, yfov=1.2, aspect=W / H)]
    fresh = []
    for cam in cams:
        d = gpu.DeviceScene(dataclasses.replace(sc, camera=cam))
        fresh.append(d.run_raytracer(W, H, SPP, seed=SEED, packet_mode=gpu.RT_PACKET_OFF)[0])
        d.close()
    assert not np.array_equal(fresh[0], fresh[1]) and not np.array_equal(fresh[1], fresh[2])
    dev = gpu.DeviceScene(sc)
    try:
        assert copy_is_made(dev, W * H * SPP)
        for v in (0, 1, 2, 1, 0, 0):
            fb, st = dev.run_raytracer_views(W, H, SPP, [cams[v]], [SEED], packet_mode=gpu.RT_PACKET_ON)
            assert st["packet_passes"] == st["passes"] == 1
            assert np.array_equal(bits(fb[0]), bits(fresh[v])), v
        own, _ = dev.run_raytracer(W, H, SPP, seed=SEED, packet_mode=gpu.RT_PACKET_ON)  # rt_render: the scene's own camera
        assert np.array_equal(bits(own), bits(fresh[0]))
    finally:
        dev.close()


@pytest.mark.parametrize("mode", ["rebuild", "rebuild_device_arrays", "refit"])
def test_new_geometry_gets_a_new_copy(gpu, scenes, mode):
    """Render, update the geometry, render again with the same camera: the second render is a fresh scene's of the new geometry. A rebuild
    swaps the binary tree under the kept copy (from host arrays and from arrays in device memory); a refit is the wide tree's (no copy is made
    of it: its packet kernel is another one) with new material ids, after which the tree is the fresh scene's."""
    sc = scenes["room_manylights"]
    kw = dict(wide=True) if mode == "refit" else {}
    new = relight(sc) if mode == "refit" else relight(deform(sc, "wave"))
    render = dict(seed=SEED, packet_mode=gpu.RT_PACKET_ON)
    d = gpu.DeviceScene(new, **kw)
    want, _ = d.run_raytracer(W, H, SPP, **render)
    d.close()
    dev = gpu.DeviceScene(sc, **kw)
    try:
        before, _ = dev.run_raytracer(W, H, SPP, **render)
        assert not np.array_equal(before, want)
        if mode == "rebuild_device_arrays":
            import torch

            a = gpu.geometry_arrays(new)
            t = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32 if k == "material_ids" else np.float32).reshape(-1)).cuda() for k, v in a.items()}
            dev.update_geometry_device(t["positions"], t["normals"], t["texcoords"], t["tangents"], t["material_ids"])
        else:
            dev.update_geometry(new, refit=(mode == "refit"))
        after, st = dev.run_raytracer(W, H, SPP, **render)
        assert st["packet_passes"] == 1
        assert np.array_equal(bits(after), bits(want)), f"{mode}: {int((bits(after) != bits(want)).any(axis=2).sum())} pixels differ from the fresh scene"
        dev.update_geometry(sc, refit=(mode == "refit"))
        back, _ = dev.run_raytracer(W, H, SPP, **render)
        assert np.array_equal(bits(back), bits(before))
    finally:
        dev.close()


def test_several_views_stay_absolute(gpu, oracle, sg, scenes):
    """Three views in one call have three origins in one queue: the pass walks the tree's own records, packets on, and every view is the
    oracle's; a single-view call in between (which makes a copy) changes nothing about the next batch."""
    sc = scenes["room_textured"]
    p = np.asarray(sc.camera.position, dtype=np.float32)
    cams = [sc.camera, sg.look_camera(p, yaw_deg=25.0, yfov=0.7, aspect=W / H), sg.look_camera(p + np.float32(0.1), yaw_deg=-40.0, yfov=1.2, aspect=W / H)]
    seeds = [11, 2024, 7]
    want = []
    for cam, seed in zip(cams, seeds):
        orc = oracle.OracleScene(dataclasses.replace(sc, camera=cam))
        want.append(orc.run_raytracer(W, H, SPP, seed=seed)[0])
        orc.close()
    dev = gpu.DeviceScene(sc)
    try:
        for _ in range(2):
            on, st = dev.run_raytracer_views(W, H, SPP, cams, seeds, packet_mode=gpu.RT_PACKET_ON)
            off, _ = dev.run_raytracer_views(W, H, SPP, cams, seeds, packet_mode=gpu.RT_PACKET_OFF)
            assert st["packet_passes"] == st["passes"]
            for v in range(3):
                assert np.array_equal(bits(on[v]), bits(want[v])) and np.array_equal(bits(off[v]), bits(want[v])), v
            dev.run_raytracer_views(W, H, SPP, [cams[1]], [seeds[1]], packet_mode=gpu.RT_PACKET_ON)
    finally:
        dev.close()


def test_caller_rays_stay_absolute(gpu, oracle, scenes):
    """rt_render_rays with packets on: rays from anywhere, after a camera render has left a copy behind. The oracle's values and counters."""
    sc = scenes["room_manylights"]
    rays = random_rays(sc, 1500, seed=5)
    dev, orc = gpu.DeviceScene(sc), oracle.OracleScene(sc)
    try:
        want, ost = orc.trace_rays(rays, samples=2, seed=SEED)
        dev.run_raytracer(W, H, SPP, seed=SEED, packet_mode=gpu.RT_PACKET_ON)
        for pkt in (gpu.RT_PACKET_ON, gpu.RT_PACKET_OFF):
            out, st = dev.render_rays(rays, samples=2, seed=SEED, counters=True, packet_mode=pkt)
            assert np.array_equal(bits(out), bits(oracle.fold_outputs([want[:, 0], want[:, 1]]))), pkt
            for k in COUNTERS:
                assert st[k] == ost[k], (k, pkt, st[k], ost[k])
        cam_rays = np.concatenate([np.tile(np.asarray(sc.camera.position, dtype=np.float32), (len(rays), 1)), rays[:, 3:]], axis=1)
        want_cam, _ = orc.trace_rays(cam_rays, samples=1, seed=SEED)  # even rays that do start at the camera: the host cannot know
        out_cam, _ = dev.render_rays(cam_rays, samples=1, seed=SEED, packet_mode=gpu.RT_PACKET_ON)
        assert np.array_equal(bits(out_cam), bits(want_cam[:, 0]))
    finally:
        dev.close()
        orc.close()


def test_accumulator_pass(gpu, sg, scenes):
    """An accumulator's passes are camera rays of its one view: packets on (the copy, for the accumulator's own camera) equal packets off,
    image and sample counts, and equal the render of that view."""
    sc = scenes["room_textured"]
    cam = sg.look_camera(np.asarray(sc.camera.position, dtype=np.float32) + np.float32(0.5), yaw_deg=15.0, yfov=0.8, aspect=W / H)
    dev = gpu.DeviceScene(sc)
    try:
        states = []
        for pkt in (gpu.RT_PACKET_ON, gpu.RT_PACKET_OFF):
            acc = dev.accumulator(W, H, camera=cam, seed=SEED)
            st = acc.render(SPP, packet_mode=pkt)
            assert st["packet_passes"] == (st["passes"] if pkt == gpu.RT_PACKET_ON else 0)
            dev.run_raytracer(W, H, SPP, seed=SEED, packet_mode=gpu.RT_PACKET_ON)  # the scene's own camera in between: another copy
            acc.render(SPP, packet_mode=pkt)
            states.append((acc.image(), acc.read()))
            acc.close()
        (img_on, r_on), (img_off, r_off) = states
        assert np.array_equal(bits(img_on), bits(img_off))
        for k in ("sum", "even_sum", "samples"):
            assert r_on[k].tobytes() == r_off[k].tobytes(), k
        assert np.all(r_on["samples"] == 2 * SPP)
        view, _ = dev.run_raytracer_views(W, H, 2 * SPP, [cam], [SEED], packet_mode=gpu.RT_PACKET_OFF)
        assert np.array_equal(bits(img_on), bits(view[0]))
    finally:
        dev.close()
