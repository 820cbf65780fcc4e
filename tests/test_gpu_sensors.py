"""GPU tests of the sensor models (include/rt_abi.h rt_sensor): rt_render_sensors*, rt_sensor_rays, rt_accum_create_sensor and the CLI.

The pins: the rays the device makes are, bit for bit, the float32 restatement of the rule (tests/sensor_replay.py, anchored without a GPU in
tests/test_sensor_replay.py); an image through a sensor is rt_render_rays over those rays and the oracle's trace_rays of them; a pinhole
sensor is rt_render_views. The base shape is 15 x 13 x 3: 585 paths per view, no multiple of 64, so the last wave and packet are partial and
a wave of a multi-sensor call straddles two sensors. All comparisons are on uint32 views."""
import ctypes as C
import importlib
import os
import subprocess
import types

import numpy as np
import pytest

import denoise_replay as dr
import feature_replay as fr
import sensor_replay as sr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 8  # RT_*
W, H, SPP = 15, 13, 3
SEED = 7
KINDS = list(sr.KIND_NAMES)
COUNTERS = ("samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests",
            "light_tri_tests", "light_hits", "texel_fetches")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _raw(rays):
    """RAY_DTYPE records as (n, 8) words"""
    return np.ascontiguousarray(rays).view(np.uint32).reshape(-1, 8)


def make_sensor(rt, cam, kind, seed=SEED):
    return {
        "pinhole": lambda: rt.Sensor.pinhole(cam, seed=seed),
        "equirect": lambda: rt.Sensor.equirect(cam, seed=seed),
        "fisheye": lambda: rt.Sensor.fisheye(cam, seed=seed),
        "orthographic": lambda: rt.Sensor.orthographic(cam, half_width=1.5, seed=seed),
        "thin_lens": lambda: rt.Sensor.thin_lens(cam, lens_radius=0.05, focus_distance=2.5, seed=seed),
    }[kind]()


@pytest.fixture(scope="module")
def abi():
    return importlib.import_module("raytracing-course-hw-public_amd._ctypes_abi")


@pytest.fixture(scope="module")
def replay(gpu, oracle, scenes):
    """(scene name, kind, spp) -> the sensor and the model's rays at W x H; computed once, shared, never written to."""
    cache = {}

    def get(name, kind, spp=SPP):
        key = (name, kind, spp)
        if key not in cache:
            sn = make_sensor(gpu, scenes[name].camera, kind)
            rays = sr.sensor_rays(oracle, sn, W, H, spp)
            rays.setflags(write=False)
            cache[key] = (sn, rays)
        return cache[key]

    return get


@pytest.fixture(scope="module")
def devs(gpu, scenes):
    d = {name: gpu.DeviceScene(scenes[name]) for name in ("room_textured", "boxes")}
    yield d
    for v in d.values():
        v.close()


# ------------------------------------------------------------------------------------------------ 1: the rays
@pytest.mark.parametrize("kind", KINDS)
def test_sensor_rays_equal_the_replay(gpu, devs, replay, abi, kind):
    import torch

    dev = devs["room_textured"]
    sn, want = replay("room_textured", kind)
    got = dev.sensor_rays(sn, W, H, SPP)
    assert got.dtype == abi.RAY_DTYPE and len(got) == W * H * SPP
    assert np.array_equal(_raw(got), _raw(want)), kind
    # a sub-range is the slice: samples 1..2 of pixels 37..136
    sub = dev.sensor_rays(sn, W, H, 2, first_pixel=37, n_pixels=100, first_sample=1)
    sel = _raw(want).reshape(W * H, SPP, 8)[37:137, 1:3].reshape(-1, 8)
    assert np.array_equal(_raw(sub), sel), kind
    # a device buffer receives the same bytes
    buf = torch.zeros(W * H * SPP * 8, dtype=torch.int32, device=f"cuda:{dev._device}")
    torch.cuda.synchronize()
    assert dev.sensor_rays(sn, W, H, SPP, device_out=buf.data_ptr()) is None
    assert np.array_equal(buf.cpu().numpy().view(np.uint32).reshape(-1, 8), _raw(want)), kind


# ------------------------------------------------------------------------------------------------ 2: sensor == rays == oracle
@pytest.mark.parametrize("name", ["room_textured", "boxes"])
@pytest.mark.parametrize("kind", KINDS)
def test_sensor_equals_rays_equals_oracle(gpu, oracle, scenes, devs, replay, kind, name):
    dev = devs[name]
    sn, rays = replay(name, kind)
    img, st = dev.render_sensors(W, H, SPP, [sn], counters=True)
    assert img.shape == (1, H, W, 3)
    orc = oracle.OracleScene(scenes[name])
    per_sample, ost = orc.trace_rays(rays, 1, seed=SEED)
    orc.close()
    want = oracle.fold_outputs(per_sample, SPP)
    assert np.array_equal(_bits(img.reshape(-1, 3)), _bits(want)), (kind, name)
    via_rays, rst = dev.render_rays(dev.sensor_rays(sn, W, H, SPP), samples=1, rays_per_output=SPP, seed=SEED, counters=True)
    assert np.array_equal(_bits(img.reshape(-1, 3)), _bits(via_rays)), (kind, name)
    for k in COUNTERS:
        assert st[k] == ost[k] == rst[k], (kind, name, k, st[k], ost[k], rst[k])
    assert np.count_nonzero(np.any(img.reshape(-1, 3) != 0, axis=1)) * 2 >= W * H


# ------------------------------------------------------------------------------------------------ 3: pinhole == views; mixed calls
def test_pinhole_equals_views_and_mixed_kinds_stack(gpu, scenes, devs):
    dev = devs["room_textured"]
    cam = scenes["room_textured"].camera
    pin, pst = dev.render_sensors(W, H, SPP, [make_sensor(gpu, cam, "pinhole")], counters=True)
    views, vst = dev.run_raytracer_views(W, H, SPP, [cam], [SEED], counters=True)
    assert np.array_equal(_bits(pin), _bits(views))
    for k in COUNTERS:
        assert pst[k] == vst[k], k
    sensors = [make_sensor(gpu, cam, kind, seed=SEED + i) for i, kind in enumerate(KINDS)]
    together, _ = dev.render_sensors(W, H, SPP, sensors)
    assert together.shape == (5, H, W, 3)
    for i, sn in enumerate(sensors):  # 585 paths per view: the waves at the seams hold two kinds
        single, _ = dev.render_sensors(W, H, SPP, [sn])
        assert np.array_equal(_bits(together[i]), _bits(single[0])), KINDS[i]
    # two pinhole sensors are two views
    cam2 = scenes["boxes"].camera
    two, _ = dev.render_sensors(W, H, SPP, [gpu.Sensor.pinhole(cam, seed=3), gpu.Sensor.pinhole(cam2, seed=4)])
    vv, _ = dev.run_raytracer_views(W, H, SPP, [cam, cam2], [3, 4])
    assert np.array_equal(_bits(two), _bits(vv))


# ------------------------------------------------------------------------------------------------ 4: scheduling independence
@pytest.mark.parametrize("kind", KINDS)
def test_scheduling_changes_no_bit(gpu, devs, replay, kind):
    dev = devs["room_textured"]
    sn, _ = replay("room_textured", kind)
    base, st = dev.render_sensors(W, H, SPP, [sn], packet_mode=gpu.RT_PACKET_OFF)
    assert st["passes"] == 1 and st["packet_passes"] == 0
    split, _ = dev.render_sensors(W, H, SPP, [sn], max_paths=256)
    assert np.array_equal(_bits(split), _bits(base)), kind
    # max_paths has a floor of 1024 paths and the base shape has 585: at 16 SPP (3120 paths) the samples split into passes of 5, 5, 5 and 1,
    # which meet through the running sum
    whole, _ = dev.render_sensors(W, H, 16, [sn], packet_mode=gpu.RT_PACKET_OFF)
    split, st = dev.render_sensors(W, H, 16, [sn], max_paths=256, packet_mode=gpu.RT_PACKET_OFF)
    assert st["passes"] == 4
    assert np.array_equal(_bits(split), _bits(whole)), kind
    split, st = dev.render_sensors(W, H, 16, [sn], max_paths=256, packet_mode=gpu.RT_PACKET_ON)
    assert st["passes"] == 4 and st["packet_passes"] == 4
    assert np.array_equal(_bits(split), _bits(whole)), kind
    srt, _ = dev.render_sensors(W, H, SPP, [sn], sort_mode=gpu.RT_SORT_OCTANT_CELL_CONE)
    assert np.array_equal(_bits(srt), _bits(base)), kind
    on, st = dev.render_sensors(W, H, SPP, [sn], packet_mode=gpu.RT_PACKET_ON)
    assert st["packet_passes"] == 1 and np.array_equal(_bits(on), _bits(base)), kind
    # 40 x 36 x 16: 23040 paths, enough (16 bytes of records per path) for the camera-relative records, which the kinds whose rays share
    # one origin then walk under RT_PACKET_ON; the film and lens kinds keep the absolute records
    dump = dev.bvh_device_dump(0)
    assert 64 * len(dump["nodes"]) + 48 * len(dump["tris"]) <= 16 * 40 * 36 * 16
    off16, _ = dev.render_sensors(40, 36, 16, [sn], packet_mode=gpu.RT_PACKET_OFF)
    on16, st = dev.render_sensors(40, 36, 16, [sn], packet_mode=gpu.RT_PACKET_ON)
    assert st["packet_passes"] == 1 and st["packet_lanes_x100"] > 0
    assert np.array_equal(_bits(on16), _bits(off16)), kind
    auto16, _ = dev.render_sensors(40, 36, 16, [sn])
    assert np.array_equal(_bits(auto16), _bits(off16)), kind


# ------------------------------------------------------------------------------------------------ 5: the other trees
@pytest.mark.parametrize("tree", ["global_best", "wide"])
def test_other_trees_equal_their_own_render_rays(gpu, scenes, tree):
    """The wide contract allows closer hits than the oracle's: the comparison is with the scene's own rt_render_rays."""
    sc = scenes["room_textured"]
    dev = gpu.DeviceScene(sc, wide=True, device_bvh=True) if tree == "wide" else gpu.DeviceScene(sc)
    gb = tree == "global_best"
    for kind in KINDS:
        sn = make_sensor(gpu, sc.camera, kind)
        img, _ = dev.render_sensors(W, H, SPP, [sn], global_best=gb)
        want, _ = dev.render_rays(dev.sensor_rays(sn, W, H, SPP), samples=1, rays_per_output=SPP, seed=SEED, global_best=gb)
        assert np.array_equal(_bits(img.reshape(-1, 3)), _bits(want)), (tree, kind)
        assert np.count_nonzero(np.any(want != 0, axis=1)) * 2 >= W * H
    dev.close()


# ------------------------------------------------------------------------------------------------ 6: accumulators
def _images_by_count(dev, sn, counts):
    return {int(n): dev.render_sensors(W, H, int(n), [sn])[0][0] for n in np.unique(counts) if n > 0}


@pytest.mark.parametrize("kind", ["equirect", "thin_lens"])
def test_accumulator_equals_render_sensors(gpu, devs, replay, kind):
    dev = devs["room_textured"]
    sn, _ = replay("room_textured", kind)
    acc = dev.accumulator(W, H, sensor=sn)
    acc.render(2)
    acc.render(3)
    want, _ = dev.render_sensors(W, H, 5, [sn])
    assert np.all(acc.read()["samples"] == 5)
    assert np.array_equal(_bits(acc.image()), _bits(want[0])), kind
    acc.close()
    # adaptive with a small cap: the threshold is a high quantile of the two-sample errors, so that the counts end up mixed
    probe = dev.accumulator(W, H, sensor=sn)
    probe.render(2)
    probe.render_adaptive(1e30, min_samples=2, max_samples=6, step=2)  # judges, adds nothing
    err = probe.read()["error"]
    assert np.all(probe.read()["samples"] == 2) and np.isfinite(err).any()
    probe.close()
    thr = float(np.quantile(err[np.isfinite(err)], 0.97))
    acc = dev.accumulator(W, H, sensor=sn)
    acc.render_adaptive(thr, min_samples=2, max_samples=6, step=2)
    n = acc.read()["samples"]
    print(f"{kind}: adaptive counts {dict(zip(*[a.tolist() for a in np.unique(n, return_counts=True)]))} at threshold {thr:.4g}")
    assert n.min() >= 2 and n.max() <= 6 and len(np.unique(n)) >= 2
    img = acc.image()
    by_n = _images_by_count(dev, sn, n)
    want = np.zeros_like(img)
    for k, im in by_n.items():
        want[n == k] = im[n == k]
    assert np.array_equal(_bits(img), _bits(want)), kind
    acc.close()


@pytest.mark.parametrize("kind", ["equirect", "thin_lens"])
def test_accumulator_features_and_denoise(gpu, oracle, scenes, devs, kind):
    N = 5
    sc = scenes["room_textured"]
    dev = devs["room_textured"]
    sn = make_sensor(gpu, sc.camera, kind)
    rays = dev.sensor_rays(sn, W, H, N)  # == the replay (test 1): sample s of pixel p, pixel-major
    od = np.concatenate([rays["origin"], rays["dir"]], axis=1).astype(np.float32)
    prim, bct = dev.cast_rays(od)
    hit = (prim != 0xFFFFFFFF).reshape(W * H, N)
    t = np.where(hit, bct[:, 2].reshape(W * H, N), np.float32(0)).astype(np.float32)
    _, _, _, shn = dev.surface_normals(od)
    assert fr.twin_alpha_is_one(sc)
    tw = oracle.OracleScene(fr.twin_scene(sc))
    albedo, _ = tw.trace_rays(rays, 1, seed=SEED)  # (n, 1, 3): colour x texel of the first hit, 0 on a miss
    tw.close()
    Z, Hn, NS, A = fr.ladder(t), fr.hit_ladder(hit), fr.ladder(shn.reshape(W * H, N, 3)), fr.ladder(albedo.reshape(W * H, N, 3))
    assert hit.any()
    acc = dev.accumulator(W, H, sensor=sn, features=True)
    total = 0
    for k in (2, 3):
        acc.render(k)
        total += k
        n = acc.read()["samples"]
        assert np.all(n == total)
        f = acc.read_features()
        assert np.array_equal(f["hits"], fr.at(Hn, n).reshape(H, W)), (kind, total)
        fr.assert_bits(f["depth_sum"], fr.at(Z, n), f"{kind} ZS after {total}")
        fr.assert_bits(f["normal_sum"], fr.at(NS, n), f"{kind} NS after {total}")
        fr.assert_bits(f["albedo_sum"], fr.at(A, n), f"{kind} AS after {total}")
    want, _ = dev.render_sensors(W, H, N, [sn])
    assert np.array_equal(_bits(acc.image()), _bits(want[0]))  # the image is the plain accumulator's
    if kind == "thin_lens":
        fr.assert_bits(acc.denoise(), dr.of_accumulator(acc), "thin_lens denoise")
    acc.close()


@pytest.mark.parametrize("features", [False, True])
def test_camera_and_pinhole_sensor_accumulators_are_one_path(gpu, scenes, devs, features):
    """An accumulator made of {camera, seed} and one made of Sensor.pinhole(camera, seed) hold the same bits after the same calls: a uniform
    render, an adaptive render whose threshold (1e-6, far below any two-sample error of a lit pixel) keeps pixels active through a second
    round, and one more uniform render."""
    dev = devs["room_textured"]
    cam = scenes["room_textured"].camera
    accs = [dev.accumulator(W, H, camera=cam, seed=SEED, features=features), dev.accumulator(W, H, sensor=gpu.Sensor.pinhole(cam, seed=SEED), features=features)]
    rounds = []
    for acc in accs:
        acc.render(SPP)
        rounds.append(acc.render_adaptive(1e-6, min_samples=SPP + 1, max_samples=SPP + 5, step=2)["rounds"])
        acc.render(3)
    assert rounds[0] == rounds[1] and rounds[0] >= 2, rounds
    a, b = accs[0].read(), accs[1].read()
    assert a["samples"].min() >= SPP + 4 and a["samples"].max() <= SPP + 8
    for k in ("sum", "even_sum", "samples", "error"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(_bits(accs[0].image()), _bits(accs[1].image()))
    if features:
        fa, fb = accs[0].read_features(), accs[1].read_features()
        for k in ("albedo_sum", "normal_sum", "depth_sum", "hits"):
            assert np.array_equal(_bits(fa[k]), _bits(fb[k])), k
    for acc in accs:
        acc.close()


# ------------------------------------------------------------------------------------------------ 7: rgb8 and device output
def test_rgb8_and_device_framebuffer(gpu, scenes, devs):
    import torch

    dev = devs["room_textured"]
    cam = scenes["room_textured"].camera
    sensors = [make_sensor(gpu, cam, "equirect"), make_sensor(gpu, cam, "orthographic")]
    fb, _ = dev.render_sensors(W, H, SPP, sensors)
    img, _ = dev.render_sensors(W, H, SPP, sensors, rgb8=True)
    assert img.dtype == np.uint8 and np.array_equal(img, gpu.tonemap(fb))
    buf = torch.zeros(2 * W * H * 3, dtype=torch.float32, device=f"cuda:{dev._device}")
    torch.cuda.synchronize()
    none, _ = dev.render_sensors(W, H, SPP, sensors, device_out=buf.data_ptr())
    assert none is None and np.array_equal(_bits(buf.cpu().numpy().reshape(2, H, W, 3)), _bits(fb))
    b8 = torch.zeros(2 * W * H * 3, dtype=torch.uint8, device=f"cuda:{dev._device}")
    torch.cuda.synchronize()
    dev.render_sensors(W, H, SPP, sensors, rgb8=True, device_out=b8.data_ptr())
    assert np.array_equal(b8.cpu().numpy().reshape(2, H, W, 3), img)


# ------------------------------------------------------------------------------------------------ 8: rt_render is untouched
def test_rt_render_is_untouched_by_sensor_calls(gpu, scenes):
    sc = scenes["room_textured"]
    dev = gpu.DeviceScene(sc)
    before, bst = dev.run_raytracer(64, 48, 16, seed=SEED)
    for kind in KINDS:  # same image shape and SPP as the render: the census of a panorama lands in the sensors' own policy
        dev.render_sensors(64, 48, 16, [make_sensor(gpu, sc.camera, kind)])
    dev.render_sensors(64, 48, 16, [make_sensor(gpu, sc.camera, k) for k in ("equirect", "orthographic")])
    after, ast = dev.run_raytracer(64, 48, 16, seed=SEED)
    assert np.array_equal(_bits(before), _bits(after))
    assert (bst["passes"], bst["packet_passes"]) == (ast["passes"], ast["packet_passes"])
    dev.close()


# ------------------------------------------------------------------------------------------------ 9: refusals
def test_refusals(gpu, abi, scenes, devs):
    lib = gpu.lib()
    dev = devs["boxes"]
    cam = scenes["boxes"].camera
    good = make_sensor(gpu, cam, "equirect")
    want, _ = dev.render_sensors(W, H, SPP, [good])
    fb = np.zeros((2, H, W, 3), dtype=np.float32)
    out = fb.ctypes.data_as(C.c_void_p)

    def params(**kw):
        p = abi.RtParams(W, H, SPP, gpu.RT_RNG_DEVICE, 0, 0, 1, 0, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def rec(name="equirect", **kw):
        r = gpu.make_sensors([make_sensor(gpu, cam, name)])
        for k, v in kw.items():
            if k == "reserved":
                r[0].reserved[v] = 1
            elif k == "fov_x":
                r[0].camera.fov_x = v
            else:
                setattr(r[0], k, v)
        return r

    def render(p, r, n=1, dst=out):
        return lib.rt_render_sensors(dev._h, C.byref(p) if p is not None else None, r, n, dst, None)

    nan, inf = float("nan"), float("inf")
    invalid = [
        ("no sensor", lambda: render(params(), rec(), 0)),
        ("null sensors", lambda: render(params(), None)),
        ("null params", lambda: render(None, rec())),
        ("null buffer", lambda: render(params(), rec(), 1, None)),
        ("unknown kind", lambda: render(params(), rec(kind=5))),
        ("reserved word", lambda: render(params(), rec(reserved=0))),
        ("last reserved word", lambda: render(params(), rec(reserved=4))),
        ("ortho half_width 0", lambda: render(params(), rec("orthographic", half_width=0.0))),
        ("ortho half_width < 0", lambda: render(params(), rec("orthographic", half_width=-1.0))),
        ("ortho half_width nan", lambda: render(params(), rec("orthographic", half_width=nan))),
        ("ortho half_width inf", lambda: render(params(), rec("orthographic", half_width=inf))),
        ("lens_radius < 0", lambda: render(params(), rec("thin_lens", lens_radius=-0.5))),
        ("lens_radius nan", lambda: render(params(), rec("thin_lens", lens_radius=nan))),
        ("focus_distance 0", lambda: render(params(), rec("thin_lens", focus_distance=0.0))),
        ("focus_distance inf", lambda: render(params(), rec("thin_lens", focus_distance=inf))),
        ("fisheye corner past 180 degrees", lambda: render(params(), rec("fisheye", fov_x=5.0))),  # 2.5 * sqrt(1 + (13/15)^2) = 3.31 > pi
        ("fisheye fov 0", lambda: render(params(), rec("fisheye", fov_x=0.0))),
        ("2^31 pixels", lambda: render(params(width=65536, height=32768), rec())),
        ("shard_count 2", lambda: render(params(shard_count=2), rec())),
        ("samples 0", lambda: render(params(samples=0), rec())),
        ("unknown flag", lambda: render(params(flags=1 << 10), rec())),
        ("sort_mode 99", lambda: render(params(sort_mode=99), rec())),
        ("packet_mode 7", lambda: render(params(packet_mode=7), rec())),
    ]
    for what, call in invalid:
        assert call() == INVALID_ARG, what
    assert render(params(), rec("fisheye", fov_x=4.0)) == OK  # 2.0 * 1.323 = 2.65 <= pi: every pixel is alive
    assert render(params(), rec("orthographic", half_width=5.0, lens_radius=nan, focus_distance=-1.0)) == OK  # fields a kind does not read are ignored
    unsupported = [
        ("reference RNG", lambda: render(params(rng_mode=gpu.RT_RNG_REFERENCE), rec())),
        ("megakernel", lambda: render(params(flags=gpu.RT_FLAG_MEGAKERNEL), rec())),
    ]
    for what, call in unsupported:
        assert call() == UNSUPPORTED, what
    # rt_sensor_rays
    rays = np.zeros(W * H * SPP, dtype=abi.RAY_DTYPE)
    rp = rays.ctypes.data_as(C.c_void_p)
    sray = lambda r, w, h, p0, np_, s0, ns, flags, dst: lib.rt_sensor_rays(dev._h, r, w, h, p0, np_, s0, ns, flags, dst)
    assert sray(rec(), W, H, 100, 96, 0, 1, 0, rp) == INVALID_ARG  # 196 > 195 pixels
    assert sray(rec(), 65535, 32768, 0, 1 << 30, 0, 2, 0, rp) == INVALID_ARG  # 2^31 records
    assert sray(rec(), W, H, 0, 10, 0, 1, gpu.RT_FLAG_COUNTERS, rp) == INVALID_ARG
    assert sray(rec(), W, H, 0, 10, 0, 1, gpu.RT_FLAG_DEVICE_FB, C.c_void_p(0x1004)) == INVALID_ARG  # misaligned: refused before any use
    assert sray(rec(), W, H, 0, 10, 0, 1, 0, None) == INVALID_ARG
    assert sray(None, W, H, 0, 10, 0, 1, 0, rp) == INVALID_ARG
    assert sray(rec(kind=9), W, H, 0, 10, 0, 1, 0, rp) == INVALID_ARG
    assert sray(rec(), 0, H, 0, 0, 0, 1, 0, rp) == INVALID_ARG
    assert sray(rec(), W, H, 0, 0, 0, 1, 0, None) == OK and sray(rec(), W, H, 195, 0, 0, 0, 0, None) == OK  # nothing to write
    # rt_accum_create_sensor
    h = C.c_void_p()
    assert lib.rt_accum_create_sensor(dev._h, W, H, rec(kind=5), 0, C.byref(h)) == INVALID_ARG and not h
    assert lib.rt_accum_create_sensor(dev._h, W, H, rec(), 2, C.byref(h)) == INVALID_ARG and not h
    assert lib.rt_accum_create_sensor(dev._h, W, H, None, 0, C.byref(h)) == INVALID_ARG and not h
    assert lib.rt_accum_create_sensor(dev._h, 0, H, rec(), 0, C.byref(h)) == INVALID_ARG and not h
    # a multi-GPU scene (two replicas on GPU 0 over the rehearsal transport)
    grp = gpu.DeviceScene(scenes["boxes"], device=[0, 0], build_flags=gpu.RT_BUILD_GROUP_COPY)
    assert lib.rt_render_sensors(grp._h, C.byref(params()), rec(), 1, out, None) == UNSUPPORTED
    assert lib.rt_sensor_rays(grp._h, rec(), W, H, 0, 10, 0, 1, 0, rp) == UNSUPPORTED
    assert lib.rt_accum_create_sensor(grp._h, W, H, rec(), 0, C.byref(h)) == UNSUPPORTED and not h
    grp.close()
    again, _ = dev.render_sensors(W, H, SPP, [good])
    assert np.array_equal(_bits(again), _bits(want))  # the scene renders what it rendered before


# ------------------------------------------------------------------------------------------------ 10: the CLI
def test_cli_camera_switches(gpu, oracle, tmp_path):
    path = os.path.join(HERE, "golden", "features", "features.gltf")
    run = os.path.join(ROOT, "run.sh")
    out = tmp_path / "pano.ppm"
    env = dict(os.environ, RT_DEVICE="0", RT_SEED="5")
    subprocess.check_call([run, path, "32", "16", "4", str(out)], env=dict(env, RT_CAMERA="equirect"))
    ls = gpu.parse_gltf_scene(path, 32 / 16)
    cam = types.SimpleNamespace(**ls.arrays()["camera"])
    dev = gpu.DeviceScene(ls)
    want, _ = dev.render_sensors(32, 16, 4, [gpu.Sensor.equirect(cam, seed=5)], rgb8=True)
    assert np.array_equal(oracle.read_ppm(str(out)), want[0])
    # thin lens through an adaptive, denoising accumulator: the accumulator of that sensor
    out2 = tmp_path / "lens.ppm"
    subprocess.check_call([run, path, "32", "16", "6", str(out2)],
                          env=dict(env, RT_CAMERA="thinlens", RT_LENS_RADIUS="0.1", RT_FOCUS_DISTANCE="3", RT_CAMERA_FOV_DEG="50", RT_ADAPTIVE="0.05",
                                   RT_ADAPTIVE_MIN="2", RT_ADAPTIVE_STEP="2", RT_DENOISE="1"))
    cam50 = types.SimpleNamespace(**dict(ls.arrays()["camera"], fov_x=np.float32(50.0) * np.float32(np.float32(3.14159265358979323846) / np.float32(180.0))))
    acc = dev.accumulator(32, 16, sensor=gpu.Sensor.thin_lens(cam50, 0.1, 3.0, seed=5), features=True)
    acc.render_adaptive(np.float32(0.05), min_samples=2, max_samples=6, step=2)
    assert np.array_equal(oracle.read_ppm(str(out2)), acc.denoise(rgb8=True))
    acc.close()
    dev.close()
    r = subprocess.run([run, path, "32", "16", "1", str(out)], env=dict(env, RT_CAMERA="hexagonal"), capture_output=True, text=True)
    assert r.returncode == 1 and "RT_CAMERA" in r.stderr
    # unset: today's path, byte for byte the golden PPM of the reference binary
    out3 = tmp_path / "plain.ppm"
    subprocess.check_call([run, path, "64", "48", "4", str(out3)], env=dict(os.environ, RT_DEVICE="0", RT_RNG_MODE="reference"))
    assert out3.read_bytes() == open(os.path.join(HERE, "golden", "features_64x48x4.ppm"), "rb").read()
