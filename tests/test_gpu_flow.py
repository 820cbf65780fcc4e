"""Motion vectors of an accumulator on the device (include/rt_abi.h rt_accum_attach_flow). The contract is bit for bit: the four per-pixel
values are the fold, in sample order, of each sample's flow as the rule states it. The expected values come from the host model
(flow_replay.py: numpy float32, and include/rt_flowspec.h compiled on the host for the two kinds that need the restated libm), fed with the
records of rt_sensor_rays and the same scene's rt_cast_rays hits: entry points that know nothing of the layer. 48 x 36 pixels, at most 8
samples, scenes of a few hundred triangles."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import flow_replay as FR

pytestmark = pytest.mark.gpu

W, H = 48, 36
F = np.float32
KINDS = ("pinhole", "equirect", "fisheye", "orthographic", "thin_lens")
STATE = ("flow_sum", "valid", "near_flow", "near_t")


def code(rt, name):
    return {v: k for k, v in rt._ctypes_abi.ERROR_NAMES.items()}[name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def room(sg):
    return sg.room_scene(300, seed=5, n_lights=3, n_materials=5)


def deformed(sc, seed=9, scale=0.3):
    """`sc` with every vertex displaced on its own: key 1 of a deforming scene."""
    rng = np.random.default_rng(seed)
    p = np.asarray(sc.positions, dtype=F)
    return dataclasses.replace(sc, positions=(p + rng.normal(scale=scale, size=p.shape).astype(F)).astype(F))


def sensor_pair(rt, sg, cam0, kind, seed=11):
    """The accumulator's view and a moved, rotated second view of the same kind."""
    cam1 = sg.look_camera(np.asarray(cam0.position, dtype=F) + np.array([0.75, 0.25, -0.5], dtype=F), yaw_deg=-86.0, yfov=0.9)
    cam1 = dataclasses.replace(cam1, fov_x=cam0.fov_x)
    make = {"pinhole": lambda c, s: rt.Sensor.pinhole(c, seed=s), "equirect": lambda c, s: rt.Sensor.equirect(c, seed=s),
            "fisheye": lambda c, s: rt.Sensor.fisheye(c, seed=s), "orthographic": lambda c, s: rt.Sensor.orthographic(c, half_width=4.0, seed=s),
            "thin_lens": lambda c, s: rt.Sensor.thin_lens(c, lens_radius=0.05, focus_distance=6.0, seed=s)}[kind]
    return make(cam0, seed), make(cam1, seed + 88)


def probe(dev, sensor, samples):
    """The primary rays of every (pixel, sample), pixel-major, and their closest hits by the scene's own probe."""
    rays = dev.sensor_rays(sensor, W, H, samples=samples)
    prim, bct = dev.cast_rays(np.concatenate([rays["origin"], rays["dir"]], axis=1))
    return rays, prim, bct


def expected(dev, s0, s1, key0, key1, n_tri, samples, counts=None):
    """The state the rule gives after `samples` samples per pixel (counts: (H, W) samples per pixel instead), and the probe's ids (P, n)."""
    rays, prim, bct = probe(dev, s0, samples)
    X0, X1, hit = FR.points(rays, prim, bct, key0, key1, n_tri)
    dx, dy, valid = FR.sample_flow(FR.view_of(s0, W, H), FR.view_of(s1 if s1 is not None else s0, W, H), W, H, X0, X1, hit)
    shape = (W * H, samples)
    if counts is not None:
        valid = valid & (np.arange(samples)[None, :] < counts.reshape(-1, 1)).reshape(-1)
    st = FR.fold(dx.reshape(shape), dy.reshape(shape), np.ascontiguousarray(bct[:, 2]).reshape(shape), valid.reshape(shape))
    return st, prim.reshape(shape)


def assert_state(acc, want, what=""):
    got = acc.read_flow()
    for k in STATE:
        w = want[k].reshape(got[k].shape)
        assert same_bits(got[k], w), f"{what}{k} differs in {(got[k].view(np.uint32) != w.view(np.uint32)).sum()} words"


def assert_fixture_in_general_position(acc, prims, samples):
    """The probe's hits and the accumulator's RT_ID_PRIMITIVE table (K = n) name the same triangles in every pixel: otherwise the replay's
    inputs are not the hits the accumulator saw, and the fixture (not the layer) is wrong."""
    ids = acc.read_ids()
    assert (ids["other"] == 0).all()
    tab_ids, tab_cnt = ids["ids"].reshape(W * H, -1), ids["counts"].reshape(W * H, -1)
    for p in range(W * H):
        u, c = np.unique(prims[p], return_counts=True)
        got = {int(i): int(n) for i, n in zip(tab_ids[p], tab_cnt[p]) if n}
        assert got == {int(i): int(n) for i, n in zip(u, c)}, f"the fixture is wrong: pixel {p}: probe {dict(zip(u, c))}, id table {got}"
    assert (tab_cnt.sum(axis=1) == samples).all()


BUILDS = {"parity": dict(), "device": dict(device_bvh=True), "wide": dict(device_bvh=True, wide=True)}


@pytest.fixture(scope="module")
def keys(gpu, sg):
    sc0 = room(sg)
    sc1 = deformed(sc0)
    return sc0, sc1, gpu.geometry_arrays(sc0)["positions"].reshape(-1, 9), gpu.geometry_arrays(sc1)["positions"].reshape(-1, 9)


# ---- 1. static is exactly zero
@pytest.mark.parametrize("kind", KINDS)
def test_static_is_zero(gpu, sg, oracle, keys, kind):
    rt, (sc0, _, key0, _) = gpu, keys
    s0, _ = sensor_pair(rt, sg, sc0.camera, kind)
    dev = rt.DeviceScene(sc0)
    # the fixture: every hit of the oracle lies where the view's projection is defined
    rays = dev.sensor_rays(s0, W, H, samples=4)
    op, ob = oracle.OracleScene(sc0).cast_rays(np.concatenate([rays["origin"], rays["dir"]], axis=1))
    X0, _, hit = FR.points(rays, op, ob, key0, key0, sc0.n_triangles)
    assert hit.sum() > 0.9 * hit.size and FR.proj(FR.view_of(s0, W, H), W, H, X0)[2][hit].all()
    acc = dev.accumulator(W, H, sensor=s0, features=True, flow=dict(key0=sc0, key1=sc0))
    acc.render(4)
    st = acc.read_flow()
    assert (st["flow_sum"] == 0).all() and (st["near_flow"] == 0).all()
    assert np.array_equal(st["valid"], acc.read_features()["hits"]) and np.array_equal(st["valid"].reshape(-1), hit.reshape(-1, 4).sum(axis=1))
    flow, mask = acc.flow()
    assert (flow == 0).all() and same_bits(mask, (st["valid"].astype(F) / F(4)).astype(F))
    dev.close()


# ---- 2. the rule, bit for bit: a deformed key 1 and a moved, rotated second view
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("kind", KINDS)
def test_equals_the_replay(gpu, sg, keys, kind, build):
    rt, (sc0, sc1, key0, key1) = gpu, keys
    s0, s1 = sensor_pair(rt, sg, sc0.camera, kind)
    dev = rt.DeviceScene(sc0, **BUILDS[build])
    n = 4
    acc = dev.accumulator(W, H, sensor=s0, ids="primitive", id_slots=n, flow=dict(key0=sc0, key1=sc1, sensor1=s1))
    acc.render(n)
    want, prims = expected(dev, s0, s1, key0, key1, sc0.n_triangles, n)
    assert_fixture_in_general_position(acc, prims, n)
    assert (want["valid"] > 0).sum() > 0.5 * W * H and np.abs(want["flow_sum"]).max() > 1.0  # something moves
    assert_state(acc, want)
    counts = acc.read()["samples"].reshape(-1)
    for mode, name in ((FR.MEAN, "mean"), (FR.NEAREST, "nearest")):
        flow, mask = acc.flow(name)
        wf, wm = FR.resolve(want, counts, mode)
        assert same_bits(flow, wf.reshape(H, W, 2)) and same_bits(mask, wm.reshape(H, W)), name
    dev.close()


# ---- 3. the sums are a function of n alone
def test_sums_are_a_function_of_n_alone(gpu, sg, keys):
    rt, (sc0, sc1, key0, key1) = gpu, keys
    s0, s1 = sensor_pair(rt, sg, sc0.camera, "pinhole")
    dev = rt.DeviceScene(sc0, device_bvh=True, wide=True)
    kw = dict(sensor=s0, flow=dict(key0=sc0, key1=sc1, sensor1=s1))
    want, _ = expected(dev, s0, s1, key0, key1, sc0.n_triangles, 8)
    one = dev.accumulator(W, H, **kw)
    one.render(8)
    assert_state(one, want, "one call: ")
    split = dev.accumulator(W, H, **kw)
    split.render(3)
    split.render(5)
    assert_state(split, want, "3 + 5: ")
    passes = dev.accumulator(W, H, **kw)
    st = passes.render(8, max_paths=3000)  # 13824 paths: several passes, and lists cut inside the round
    assert st["passes"] > 3
    assert_state(passes, want, "max_paths: ")
    for sort_mode in (rt.RT_SORT_AUTO, rt.RT_SORT_OFF, rt.RT_SORT_OCTANT_CELL_CONE):
        for packet_mode in (rt.RT_PACKET_AUTO, rt.RT_PACKET_OFF, rt.RT_PACKET_ON):
            a = dev.accumulator(W, H, **kw)
            a.render(5, sort_mode=sort_mode, packet_mode=packet_mode)
            a.render(3, sort_mode=sort_mode, packet_mode=packet_mode, max_paths=5000)
            assert_state(a, want, f"sort {sort_mode} packet {packet_mode}: ")
            a.close()
    # unequal counts: the state is the fold of each pixel's first n_p samples
    judge = dev.accumulator(W, H, sensor=s0)  # a threshold that splits the pixels: the median error after two samples
    judge.render(2)
    judge.render_adaptive(0.0, min_samples=2, max_samples=2, step=1)
    err = judge.read()["error"]
    judge.close()
    ad = dev.accumulator(W, H, **kw)
    ad.render_adaptive(float(np.median(err[np.isfinite(err)])), min_samples=2, max_samples=8, step=3, max_paths=4000)
    counts = ad.read()["samples"]
    assert counts.min() < counts.max() <= 8
    want_ad, _ = expected(dev, s0, s1, key0, key1, sc0.n_triangles, 8, counts=counts)
    assert_state(ad, want_ad, "adaptive: ")
    flow, mask = ad.flow("mean")
    wf, wm = FR.resolve(want_ad, counts.reshape(-1), FR.MEAN)
    assert same_bits(flow, wf.reshape(H, W, 2)) and same_bits(mask, wm.reshape(H, W))
    dev.close()


# ---- 4. neutrality: every other sum, image and counter is that of an accumulator without flow
def test_flow_changes_nothing_else(gpu, sg, keys):
    rt, (sc0, sc1, _, _) = gpu, keys
    s0, s1 = sensor_pair(rt, sg, sc0.camera, "pinhole")
    n_mats = len(sc0.materials)
    layers = dict(sensor=s0, features=True, ids="material", id_slots=3, light_groups=dict(material_group=[m % 2 for m in range(n_mats)], background=1, n_groups=2))
    dev = rt.DeviceScene(sc0, device_bvh=True, wide=True)
    plain = dev.accumulator(W, H, **layers)
    with_flow = dev.accumulator(W, H, flow=dict(key0=sc0, key1=sc1, sensor1=s1), **layers)
    stats = []
    for acc in (plain, with_flow):
        a = acc.render(3, counters=True)
        b = acc.render(2, counters=True, max_paths=3000)
        stats.append((a, b))
    timing = ("kernel_ms", "total_ms", "dominant_ms")
    for x, y in zip(stats[0], stats[1]):
        assert {k: v for k, v in x.items() if k not in timing} == {k: v for k, v in y.items() if k not in timing}
    for read in ("read", "read_features", "read_ids"):
        a, b = getattr(plain, read)(), getattr(with_flow, read)()
        for name in a:
            assert same_bits(a[name], b[name]), (read, name)
    assert same_bits(plain.read_light_groups(), with_flow.read_light_groups())
    assert same_bits(plain.image(), with_flow.image()) and same_bits(plain.denoise(), with_flow.denoise())
    dev.close()


# ---- 5. n_triangles == 0: the camera's flow alone, on a scene with analytic primitives
def test_camera_only_flow_on_analytic_primitives(gpu, sg):
    from conftest import SCENE000

    rt = gpu
    ls = rt.parse_scene_txt(SCENE000)
    assert ls.desc.n_primitives > 0
    dev, cam0 = rt.DeviceScene(ls), ls.cameras()[0]
    cam1 = dataclasses.replace(cam0, position=(np.asarray(cam0.position, dtype=F) + np.array([0.25, 0.125, -0.25], dtype=F)).astype(F))
    s0, s1 = rt.Sensor.pinhole(cam0, seed=21), rt.Sensor.pinhole(cam1, seed=22)
    n = 4
    acc = dev.accumulator(W, H, sensor=s0, ids="primitive", id_slots=n, flow=dict(sensor1=s1))
    acc.render(n)
    want, prims = expected(dev, s0, s1, None, None, int(ls.desc.n_triangles), n)
    assert_fixture_in_general_position(acc, prims, n)
    assert ((prims >= ls.desc.n_triangles) & (prims != 0xFFFFFFFF)).any() and np.abs(want["flow_sum"]).max() > 0.5
    assert_state(acc, want)
    dev.close()


# ---- 6. keys in HBM and outputs in HBM equal the host path; the caller's tensors are not kept
def test_device_keys_and_device_outputs(gpu, sg, keys):
    import torch

    rt, (sc0, sc1, key0, key1) = gpu, keys
    s0, s1 = sensor_pair(rt, sg, sc0.camera, "fisheye")
    dev = rt.DeviceScene(sc0, device_bvh=True)
    host = dev.accumulator(W, H, sensor=s0, flow=dict(key0=sc0, key1=sc1, sensor1=s1))
    tens = [torch.from_numpy(k.copy()).to("cuda:0") for k in (key0, key1)]
    ondev = dev.accumulator(W, H, sensor=s0, flow=dict(key0=tens[0], key1=dict(positions=tens[1]), sensor1=s1))
    for t in tens:  # copied at attach: the caller may overwrite theirs
        t.zero_()
    torch.cuda.synchronize()
    for acc in (host, ondev):
        acc.render(3)
    a, b = host.read_flow(), ondev.read_flow()
    for k in STATE:
        assert same_bits(a[k], b[k]), k
    assert np.abs(a["flow_sum"]).max() > 1.0
    for mode in ("mean", "nearest"):
        flow, mask = host.flow(mode)
        d_flow, d_mask = torch.full((H, W, 2), -7.0, device="cuda:0"), torch.full((H, W), -7.0, device="cuda:0")
        torch.cuda.synchronize()
        assert ondev.flow(mode, device_out=(d_flow.data_ptr(), d_mask.data_ptr())) == (None, None)
        assert same_bits(d_flow.cpu().numpy(), flow) and same_bits(d_mask.cpu().numpy(), mask)
        d_flow.fill_(-7.0)
        torch.cuda.synchronize()
        ondev.flow(mode, device_out=(d_flow.data_ptr(), None))  # either output may be NULL
        assert same_bits(d_flow.cpu().numpy(), flow)
    dev.close()


# ---- 7. the refusals, each leaving everything as it was
def test_refusals(gpu, sg, keys):
    import torch

    rt, (sc0, sc1, key0, key1) = gpu, keys
    INVALID, UNSUPPORTED = code(rt, "RT_ERR_INVALID_ARG"), code(rt, "RT_ERR_UNSUPPORTED")
    lib = rt.lib()
    s0, s1 = sensor_pair(rt, sg, sc0.camera, "pinhole")
    dev = rt.DeviceScene(sc0, device_bvh=True, wide=True)
    layers = dict(sensor=s0, features=True, ids="primitive")
    plain, twin = dev.accumulator(W, H, **layers), dev.accumulator(W, H, **layers)

    def state(acc, with_flow):
        out = {**acc.read(), **acc.read_features(), **acc.read_ids()}
        if with_flow:
            out.update(acc.read_flow())
        return out

    def refused(call, err, acc, with_flow=False):
        before = state(acc, with_flow)
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == err, str(e.value)
        after = state(acc, with_flow)
        for k in before:
            assert same_bits(before[k], after[k]), k
        return str(e.value)

    def raw(acc, n=None, flags=0, k0=key0, k1=key1, sensor1=None, reserved=()):
        d = rt._ctypes_abi.RtFlowDesc()
        d.n_triangles = sc0.n_triangles if n is None else n
        d.flags = flags
        keep = [None if k is None else (k if isinstance(k, int) else np.ascontiguousarray(k, dtype=F)) for k in (k0, k1)]
        for i, k in enumerate(keep):
            d.positions[i] = None if k is None else (k if isinstance(k, int) else k.ctypes.data)
        if sensor1 is not None:
            rec = rt.make_sensors([sensor1])
            d.sensor1 = C.cast(rec, C.POINTER(rt._ctypes_abi.RtSensor))
        for i, r in enumerate(reserved):
            d.reserved[i] = r
        rt._check(lib.rt_accum_attach_flow(acc._h, C.byref(d)))

    # NULL arguments (no accumulator to compare: the call has none)
    assert lib.rt_accum_attach_flow(None, C.byref(rt._ctypes_abi.RtFlowDesc())) == INVALID and lib.rt_accum_attach_flow(plain._h, None) == INVALID
    assert lib.rt_accum_read_flow(None, None, None, None, None) == INVALID and lib.rt_accum_resolve_flow(None, 0, 0, None, None) == INVALID
    # a read or a resolve without flow
    refused(lambda: plain.read_flow(), INVALID, plain)
    refused(lambda: plain.flow(), INVALID, plain)
    # n_triangles neither 0 nor the scene's; a NULL key; an unknown flag; a reserved word
    refused(lambda: raw(plain, n=sc0.n_triangles - 1, k0=key0[:-1], k1=key1[:-1]), INVALID, plain)
    refused(lambda: raw(plain, k1=None), INVALID, plain)
    refused(lambda: raw(plain, k0=None), INVALID, plain)
    refused(lambda: raw(plain, flags=2), INVALID, plain)
    refused(lambda: raw(plain, flags=rt.RT_FLAG_DEVICE_FB | 4), INVALID, plain)
    refused(lambda: plain.attach_flow(key0=sc0, key1=sc1, reserved=[0, 0, 0, 0, 0, 0, 0, 1]), INVALID, plain)
    # a non-finite position in either key: the lowest triangle is named
    for which in (0, 1):
        bad = (key0 if which == 0 else key1).copy()
        bad[77, 4], bad[40, 2] = np.inf, np.nan
        msg = refused(lambda: raw(plain, **{f"k{which}": bad}), INVALID, plain)
        assert "triangle 40" in msg and f"key {which}" in msg
    # device arrays: misaligned, or host memory under the device flag
    t0, t1 = (torch.from_numpy(np.concatenate([k.reshape(-1), np.zeros(1, dtype=F)])).to("cuda:0") for k in (key0, key1))
    torch.cuda.synchronize()
    refused(lambda: raw(plain, flags=rt.RT_FLAG_DEVICE_FB, k0=t0.data_ptr(), k1=t1.data_ptr() + 2), INVALID, plain)
    assert "not device memory" in refused(lambda: raw(plain, flags=rt.RT_FLAG_DEVICE_FB, k0=t0.data_ptr(), k1=np.ascontiguousarray(key1).ctypes.data), INVALID, plain)
    # sensor1 of another kind, or one rt_render_sensors refuses
    refused(lambda: plain.attach_flow(key0=sc0, key1=sc1, sensor1=rt.Sensor.equirect(sc0.camera)), INVALID, plain)
    bad_sensor = rt.make_sensors([s1])
    bad_sensor[0].reserved[2] = 1
    refused(lambda: raw(plain, sensor1=bad_sensor[0]), INVALID, plain)
    # after all of that the accumulator renders what its twin renders, and still takes the layer
    plain.attach_flow(key0=sc0, key1=sc1, sensor1=s1)
    for acc in (plain, twin):
        acc.render(2)
    a, b = state(plain, False), state(twin, False)
    for k in a:
        assert same_bits(a[k], b[k]), k
    want, _ = expected(dev, s0, s1, key0, key1, sc0.n_triangles, 2)
    assert_state(plain, want)
    # a second attach, an attach after samples were added, an unknown mode or flag of the resolve
    refused(lambda: plain.attach_flow(key0=sc0, key1=sc1), INVALID, plain, True)
    refused(lambda: twin.attach_flow(key0=sc0, key1=sc1), INVALID, twin)
    refused(lambda: plain.flow(2), INVALID, plain, True)
    out = np.zeros((H, W, 2), dtype=F)
    refused(lambda: rt._check(lib.rt_accum_resolve_flow(plain._h, 0, 2, out.ctypes.data_as(C.c_void_p), None)), INVALID, plain, True)
    plain.close(), twin.close()
    # flow and a shutter, in either order (a shutter wants to be the scene's only accumulator)
    first_shutter = dev.accumulator(W, H, sensor=s0, shutter=dict(key0=sc0, key1=sc1, slices=2, block=1, refit=True))
    with pytest.raises(rt.RtError) as e:
        first_shutter.attach_flow(key0=sc0, key1=sc1)
    assert e.value.code == UNSUPPORTED
    first_shutter.render(2)
    first_shutter.close()
    first_flow = dev.accumulator(W, H, sensor=s0, flow=dict(key0=sc0, key1=sc1, sensor1=s1))
    with pytest.raises(rt.RtError) as e:
        first_flow.attach_shutter(key0=sc0, key1=sc1, slices=2, block=1, refit=True)
    assert e.value.code == UNSUPPORTED
    first_flow.render(2)
    assert_state(first_flow, expected(dev, s0, s1, key0, key1, sc0.n_triangles, 2)[0])
    dev.close()


# ---- 8. sign and convention, end to end: frame 1 sampled at p + flow(p) is frame 0
def test_warping_frame_1_by_the_flow_gives_frame_0(gpu, sg):
    rt = gpu
    u, v = np.meshgrid((np.arange(64) + 0.5) / 64, (np.arange(64) + 0.5) / 64)
    tex = np.stack([0.5 + 0.4 * np.sin(2 * np.pi * 3 * u + 1.0), 0.5 + 0.4 * np.sin(2 * np.pi * 2 * v), 0.5 + 0.4 * np.sin(2 * np.pi * (2 * u + 3 * v)), np.ones_like(u)], axis=2)
    tex = np.clip(np.round(tex * 255.0), 0, 255).astype(np.uint8)

    def scene(shift, bulge):
        # one textured diffuse quad that overfills the view, under the white background: a path leaves it after one bounce, so a pixel is its texel
        a, b, c, d = (np.array(p, dtype=F) for p in ((-12, -9, 0), (12, -9, 0), (12, 9, 0), (-12, 9, 0)))
        pos = (np.array([[a, b, c], [a, c, d]], dtype=F) + np.asarray(shift, dtype=F)).astype(F)
        pos[0, 1] += np.asarray(bulge, dtype=F)  # one corner of one triangle: the scene deforms, it does not only translate
        uv = np.array([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]], dtype=F)
        tan = np.zeros((2, 3, 3), dtype=F)
        tan[..., 0] = 1
        mats = [sg.Material(color=(1.0, 1.0, 1.0, 1.0), roughness=1.0, metallic=0.0, color_tex=0)]
        return sg.Scene(pos, None, uv, tan, np.zeros(2, dtype=np.uint32), mats, textures=[tex], camera=sg.look_camera((0.0, 0.0, 10.0), yaw_deg=0.0, yfov=0.9))

    sc0, sc1 = scene((0, 0, 0), (0, 0, 0)), scene((0.5, -0.25, 0.0), (0.0, -0.5, 0.5))
    cam1 = sg.look_camera((-0.3, 0.2, 10.5), yaw_deg=1.5, yfov=0.9)
    s0, s1 = rt.Sensor.pinhole(sc0.camera, seed=4), rt.Sensor.pinhole(dataclasses.replace(cam1, fov_x=sc0.camera.fov_x), seed=4)
    dev0, dev1 = rt.DeviceScene(sc0), rt.DeviceScene(sc1)
    acc0 = dev0.accumulator(W, H, sensor=s0, flow=dict(key0=sc0, key1=sc1, sensor1=s1))
    acc1 = dev1.accumulator(W, H, sensor=s1)
    for acc in (acc0, acc1):
        acc.render(8)
    frame0, frame1 = acc0.image().astype(np.float64), acc1.image().astype(np.float64)
    flow, mask = acc0.flow("mean")
    full = mask == 1
    assert full.sum() > 0.9 * W * H and np.abs(flow[full]).max() > 1.0
    ys, xs = np.mgrid[0:H, 0:W]
    tx, ty = np.clip(xs + flow[..., 0], 0, W - 1), np.clip(ys + flow[..., 1], 0, H - 1)
    x0, y0 = np.minimum(np.floor(tx).astype(int), W - 2), np.minimum(np.floor(ty).astype(int), H - 2)
    fx, fy = (tx - x0)[..., None], (ty - y0)[..., None]
    warped = (1 - fy) * ((1 - fx) * frame1[y0, x0] + fx * frame1[y0, x0 + 1]) + fy * ((1 - fx) * frame1[y0 + 1, x0] + fx * frame1[y0 + 1, x0 + 1])
    err_warped, err_plain = np.abs(warped - frame0)[full].mean(), np.abs(frame1 - frame0)[full].mean()
    print(f"mean absolute error against frame 0: frame 1 warped by the flow {err_warped:.5f}, frame 1 as it is {err_plain:.5f}")
    assert err_warped < err_plain
    # the opposite sign, or x and y exchanged, would not do
    for wrong in (-flow, flow[..., ::-1]):
        tx, ty = np.clip(xs + wrong[..., 0], 0, W - 1), np.clip(ys + wrong[..., 1], 0, H - 1)
        assert np.abs(frame1[np.rint(ty).astype(int), np.rint(tx).astype(int)] - frame0)[full].mean() > err_warped
    dev0.close(), dev1.close()
