"""GPU tests of rt_render_views / rt_render_views_rgb8: K camera views of one built scene in one call. View v of a batch must be, bit for
bit, the single render of a scene created with camera v and rendered with seed v, in every mode (wavefront pipeline, global-best and wide
production traversals, megakernel, reference RNG, multi-GPU group), across pass tiles that straddle views, sorted batches and shards."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from multiview import three_camera_gltf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP = 64, 48, 4
INVALID_ARG, UNSUPPORTED = 1, 8  # RT_ERR_*


def _cameras(sg, sc):
    """The scene's own camera plus two others (other yaw and fov), all from the scene camera's position."""
    p = sc.camera.position
    return [sc.camera, sg.look_camera(p, yaw_deg=25.0, yfov=0.7, aspect=W / H), sg.look_camera(p + np.float32(0.1), yaw_deg=-40.0, yfov=1.2, aspect=W / H)]


def _with_camera(sc, cam):
    return dataclasses.replace(sc, camera=cam)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


SEEDS = [11, 2024, 7]


@pytest.mark.parametrize("name", ["room_textured", "room_manylights", "boxes"])
def test_views_device_rng_match_oracle(gpu, oracle, sg, scenes, name):
    sc = scenes[name]
    cams = _cameras(sg, sc)
    dev = gpu.DeviceScene(sc)
    fb, st = dev.run_raytracer_views(W, H, SPP, cams, SEEDS, counters=True)
    assert fb.shape == (3, H, W, 3) and st["samples"] == 3 * W * H * SPP
    for v, cam in enumerate(cams):
        ofb, _ = oracle.OracleScene(_with_camera(sc, cam)).run_raytracer(W, H, SPP, rng_mode=gpu.RT_RNG_DEVICE, seed=SEEDS[v])
        assert np.array_equal(_bits(fb[v]), _bits(ofb)), (name, v)
    assert not np.array_equal(fb[0], fb[1]) and not np.array_equal(fb[1], fb[2])
    # the scene's own camera is unchanged by a batch
    single, _ = dev.run_raytracer(W, H, SPP, seed=SEEDS[0])
    assert np.array_equal(_bits(single), _bits(fb[0]))


@pytest.mark.parametrize("mode", ["reference", "megakernel"])
def test_views_reference_rng_and_megakernel_match_oracle(gpu, oracle, sg, scenes, mode):
    sc = scenes["room_textured"]
    cams = _cameras(sg, sc)
    dev = gpu.DeviceScene(sc)
    rng = gpu.RT_RNG_REFERENCE if mode == "reference" else gpu.RT_RNG_DEVICE
    fb, st = dev.run_raytracer_views(W, H, SPP, cams, SEEDS, rng_mode=rng, megakernel=(mode == "megakernel"))
    assert st["passes"] == 3  # one megakernel launch per view
    for v, cam in enumerate(cams):
        ofb, _ = oracle.OracleScene(_with_camera(sc, cam)).run_raytracer(W, H, SPP, rng_mode=rng, seed=SEEDS[v])
        assert np.array_equal(_bits(fb[v]), _bits(ofb)), (mode, v)


@pytest.mark.parametrize("flags", [dict(global_best=True), dict(device_bvh=True, wide=True)])
def test_views_production_modes_match_single_renders(gpu, sg, scenes, flags):
    sc = scenes["room_manylights"]
    cams = _cameras(sg, sc)
    build = {k: v for k, v in flags.items() if k in ("device_bvh", "wide")}
    render = {k: v for k, v in flags.items() if k == "global_best"}
    dev = gpu.DeviceScene(sc, **build)
    fb, _ = dev.run_raytracer_views(W, H, SPP, cams, SEEDS, **render)
    for v, cam in enumerate(cams):
        one = gpu.DeviceScene(_with_camera(sc, cam), **build)
        ref, _ = one.run_raytracer(W, H, SPP, seed=SEEDS[v], **render)
        assert np.array_equal(_bits(fb[v]), _bits(ref)), (flags, v)
        one.close()


def test_views_pass_tiles_straddle_views(gpu, sg, scenes):
    """max_paths 5000: two pixel tiles over the 3 x 3072-pixel virtual image (the first ends inside view 1), one sample per pass."""
    sc = scenes["room_plain"]
    cams = _cameras(sg, sc)
    dev = gpu.DeviceScene(sc)
    full, st_full = dev.run_raytracer_views(W, H, SPP, cams, SEEDS)
    assert st_full["passes"] == 1
    calls = []
    tiled, st = dev.run_raytracer_views(W, H, SPP, cams, SEEDS, max_paths=5000, progress=lambda d, t: calls.append((d, t)))
    assert st["passes"] == 2 * SPP
    assert calls == [(k, 2 * SPP) for k in range(1, 2 * SPP + 1)]
    assert np.array_equal(_bits(tiled), _bits(full))


def test_views_sorted_batch_equals_single_view_calls(gpu, sg):
    """8 views of 256 x 256 x 4 = 2^21 paths in one pass: RT_SORT_AUTO sorts the batch's bounces (a single view, 2^18 paths, runs unsorted),
    and the batch's primary rays go through the packet kernel."""
    sc = sg.room_scene(100_000, seed=41, n_lights=6, n_materials=6, tex_size=16, n_tex_sets=2)
    p = sc.camera.position
    cams = [sg.look_camera(p, yaw_deg=-60.0 + 17.0 * k, yfov=0.6 + 0.1 * k) for k in range(8)]
    seeds = [100 + k for k in range(8)]
    dev = gpu.DeviceScene(sc)
    batch, st = dev.run_raytracer_views(256, 256, 4, cams, seeds, packet_mode=gpu.RT_PACKET_ON)
    assert st["passes"] == 1 and st["packet_passes"] == 1
    for v, cam in enumerate(cams):
        one, _ = dev.run_raytracer_views(256, 256, 4, [cam], [seeds[v]])
        assert np.array_equal(_bits(batch[v]), _bits(one[0])), v
    # and a one-view batch of the scene's own camera is rt_render
    a, _ = dev.run_raytracer_views(256, 256, 4, [sc.camera], [5])
    b, _ = dev.run_raytracer(256, 256, 4, seed=5)
    assert np.array_equal(_bits(a[0]), _bits(b))


@pytest.mark.parametrize("megakernel,block", [(False, 256), (True, 256), (True, 1000)])
def test_views_shards_assemble_the_batch(gpu, sg, scenes, megakernel, block):
    sc = scenes["room_textured"]
    cams = _cameras(sg, sc)
    dev = gpu.DeviceScene(sc)
    full, _ = dev.run_raytracer_views(W, H, SPP, cams, SEEDS, megakernel=megakernel)
    n = 3 * W * H
    owner = (np.arange(n) // block) % 3
    assembled = np.full((3, H, W, 3), -7.0, dtype=np.float32)
    for r in range(3):
        part = np.full((3, H, W, 3), -7.0, dtype=np.float32)
        dev.run_raytracer_views(W, H, SPP, cams, SEEDS, shard_index=r, shard_count=3, shard_block=block, out=part, megakernel=megakernel)
        flat = part.reshape(n, 3)
        assert np.all(flat[owner != r] == -7.0), r  # other shards' pixels keep the sentinel
        assembled.reshape(n, 3)[owner == r] = flat[owner == r]
    assert np.array_equal(_bits(assembled), _bits(full))


def test_views_rgb8_host_and_device(gpu, sg, scenes):
    import torch

    sc = scenes["room_manylights"]
    cams = _cameras(sg, sc)
    dev = gpu.DeviceScene(sc)
    fb, _ = dev.run_raytracer_views(W, H, SPP, cams, SEEDS)
    img, _ = dev.run_raytracer_views(W, H, SPP, cams, SEEDS, rgb8=True)
    assert img.dtype == np.uint8 and np.array_equal(img, gpu.tonemap(fb))
    t = torch.full((3 * H * W * 3,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dev.run_raytracer_views(W, H, SPP, cams, SEEDS, rgb8=True, device_fb=t.data_ptr())
    assert np.array_equal(t.cpu().numpy().reshape(3, H, W, 3), img)
    tf = torch.zeros((3 * H * W * 3,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dev.run_raytracer_views(W, H, SPP, cams, SEEDS, device_fb=tf.data_ptr())
    assert np.array_equal(_bits(tf.cpu().numpy().reshape(3, H, W, 3)), _bits(fb))


@pytest.mark.parametrize("rng", ["device", "reference"])
def test_views_group_rehearsal(gpu, sg, scenes, rng):
    sc = scenes["room_plain"]
    cams = _cameras(sg, sc)
    mode = gpu.RT_RNG_DEVICE if rng == "device" else gpu.RT_RNG_REFERENCE
    one = gpu.DeviceScene(sc)
    want, _ = one.run_raytracer_views(W, H, SPP, cams, SEEDS, rng_mode=mode)
    grp = gpu.DeviceScene(sc, device=[0, 0, 0], build_flags=gpu.RT_BUILD_GROUP_COPY)
    assert grp.n_devices == 3
    got, st = grp.run_raytracer_views(W, H, SPP, cams, SEEDS, rng_mode=mode)
    assert np.array_equal(_bits(got), _bits(want))
    img, _ = grp.run_raytracer_views(W, H, SPP, cams, SEEDS, rng_mode=mode, rgb8=True)
    assert np.array_equal(img, gpu.tonemap(want))


def test_views_argument_checks(gpu, sg, scenes):
    import ctypes as C

    sc = scenes["room_plain"]
    cams = _cameras(sg, sc)
    dev = gpu.DeviceScene(sc)
    lib = gpu.lib()
    abi = gpu._ctypes_abi
    fb = np.zeros((3, H, W, 3), dtype=np.float32)
    views = gpu.make_views(cams, SEEDS)

    def call(p, views, n, buf=fb):
        return lib.rt_render_views(dev._h, C.byref(p), views, n, buf.ctypes.data_as(C.c_void_p) if buf is not None else None, None)

    p = abi.RtParams(W, H, SPP, gpu.RT_RNG_DEVICE, 0, 0, 1, 0, 0)
    assert call(p, views, 3) == 0
    assert call(p, views, 0) == INVALID_ARG
    assert call(p, None, 3) == INVALID_ARG
    assert call(p, views, 3, None) == INVALID_ARG
    bad = gpu.make_views(cams, SEEDS)
    bad[1].reserved = 1
    assert call(p, bad, 3) == INVALID_ARG
    big = abi.RtParams(32768, 32768, 1, gpu.RT_RNG_DEVICE, 0, 0, 1, 0, 0)  # 2^30 pixels per view, 2^31 in two views
    assert call(big, views, 2) == INVALID_ARG
    ref = abi.RtParams(W, H, SPP, gpu.RT_RNG_REFERENCE, 0, 0, 3, 256, 0)
    assert call(ref, views, 3) == INVALID_ARG
    assert call(ref, views, 1) == 0  # one view: reference-RNG shards as rt_render does
    # a wide scene refuses the megakernel and the reference RNG, as rt_render does
    wide = gpu.DeviceScene(sc, device_bvh=True, wide=True)
    for q in (abi.RtParams(W, H, SPP, gpu.RT_RNG_REFERENCE, 0, 0, 1, 0, 0), abi.RtParams(W, H, SPP, gpu.RT_RNG_DEVICE, 0, 0, 1, 0, gpu.RT_FLAG_MEGAKERNEL)):
        assert lib.rt_render_views(wide._h, C.byref(q), views, 3, fb.ctypes.data_as(C.c_void_p), None) == UNSUPPORTED
    # ray_depth == 0: a no-op that leaves the buffer untouched
    dark = gpu.DeviceScene(dataclasses.replace(sc, ray_depth=0))
    sentinel = np.full((3, H, W, 3), 3.5, dtype=np.float32)
    assert lib.rt_render_views(dark._h, C.byref(p), views, 3, sentinel.ctypes.data_as(C.c_void_p), None) == 0
    assert np.all(sentinel == 3.5)


def test_cli_all_cameras(gpu, sg, tmp_path):
    path, variants = three_camera_gltf(sg, tmp_path)
    run = os.path.join(ROOT, "run.sh")
    env = dict(os.environ, RT_SEED="9", RT_DEVICE="0")
    out = tmp_path / "all" / "img.ppm"
    subprocess.check_call([run, path, str(W), str(H), str(SPP), str(out)], env=dict(env, RT_ALL_CAMERAS="1"))
    assert sorted(os.listdir(out.parent)) == ["img_0.ppm", "img_1.ppm", "img_2.ppm"]
    for i, vp in enumerate(variants):
        single = tmp_path / f"single{i}.ppm"
        subprocess.check_call([run, vp, str(W), str(H), str(SPP), str(single)], env=env)
        assert (out.parent / f"img_{i}.ppm").read_bytes() == single.read_bytes(), i
    plain = tmp_path / "plain" / "img.ppm"
    subprocess.check_call([run, path, str(W), str(H), str(SPP), str(plain)], env=env)
    assert os.listdir(plain.parent) == ["img.ppm"]
    assert plain.read_bytes() == (out.parent / "img_2.ppm").read_bytes()  # the plain render uses the last camera, as the reference does
