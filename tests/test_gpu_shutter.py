"""Shutter accumulators on the device (include/rt_abi.h rt_accum_attach_shutter). The contract is bit for bit: sample s of pixel p is the
sample of rt_render_sensors with the sensor of its slice on a scene updated to the geometry of its slice, added in sample order. The
expected values are built from the numpy replay of the rule (shutter_replay.py) and from entry points that know nothing of a shutter:
rt_update_geometry on a second scene, rt_sensor_rays and rt_render_rays for one sample of every pixel. 32 x 24 pixels, at most 16 samples."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import shutter_replay as R

pytestmark = pytest.mark.gpu

W, H = 32, 24
F = np.float32
N_WALLS, N_LIGHTS = 12, 3  # room_scene: the walls come first, then the lights, then the random triangles


def code(rt, name):
    return {v: k for k, v in rt._ctypes_abi.ERROR_NAMES.items()}[name]


def room(sg, **kw):
    return sg.room_scene(300, seed=5, n_lights=N_LIGHTS, n_materials=5, **kw)


def moved(sc, tris, delta):
    """`sc` with the triangles `tris` translated by `delta`."""
    p = np.asarray(sc.positions, dtype=F).copy()
    p[tris] = (p[tris] + np.asarray(delta, dtype=F)).astype(F)
    return dataclasses.replace(sc, positions=p)


def keys_of(sg, lights_move=True):
    """Key 0: a small room. Key 1: a block of 100 random triangles moved by about a tenth of the room's extent, and one emissive triangle."""
    sc0 = room(sg)
    first = N_WALLS + N_LIGHTS
    sc1 = moved(sc0, slice(first + 50, first + 150), (3.5, 1.0, -2.0))
    if lights_move:
        sc1 = moved(sc1, slice(N_WALLS, N_WALLS + 1), (2.0, -0.5, 1.0))
    return sc0, sc1


def sensors_of(rt, sg, sc):
    cam0 = sc.camera
    cam1 = sg.look_camera(np.asarray(cam0.position, dtype=F) + np.array([0.75, 0.25, -0.5], dtype=F), yaw_deg=-86.0, yfov=0.9)
    return rt.Sensor.pinhole(cam0, seed=11), rt.Sensor.pinhole(dataclasses.replace(cam1, fov_x=cam0.fov_x * 1.05), seed=99)


def update_raw(rt, dev, arrays, refit):
    """rt_update_geometry of flat host arrays exactly as given (DeviceScene.update_geometry would normalise the normals of a dict again)."""
    u = rt.RtGeometryUpdate()
    u.n_triangles = arrays["material_ids"].size
    u.mode = rt.RT_UPDATE_REFIT if refit else rt.RT_UPDATE_REBUILD
    keep = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    for name in ("positions", "normals", "texcoords", "tangents"):
        setattr(u, name, rt.fptr(keep[name]))
    u.material_ids = rt.u32ptr(keep["material_ids"])
    rt._check(rt.lib().rt_update_geometry(dev._h, C.byref(u)))


def one_sample(dev, sensor, s):
    """X(p, s) for every pixel: the rays the device makes for sample s of `sensor`, path-traced one sample each."""
    rays = dev.sensor_rays(sensor, W, H, samples=1, first_sample=s)
    out, _ = dev.render_rays(rays, samples=1, seed=sensor.seed)
    return out.reshape(H, W, 3)


def expected_sums(rt, ref, key0, key1, s0, s1, n_samples, slices, block, refit, open=0.0, close=1.0):
    """(S, E) by the contract, on `ref`, a second scene of key 0 (key0 None: the geometry does not move)."""
    installed = [None]

    def sample(s):
        k = R.slice_of(s, slices, block)
        t = R.slice_time(k, slices, open, close)
        if key0 is not None and installed[0] != k:
            update_raw(rt, ref, R.geometry_at(key0, key1, t), refit)
            installed[0] = k
        return one_sample(ref, R.sensor_at(s0, s1, t), s)

    return R.accumulate(sample, n_samples, (H, W, 3))


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def assert_state(acc, S, E, n):
    st = acc.read()
    assert (st["samples"] == n).all()
    assert same_bits(st["sum"], S), f"S differs in {(st['sum'].view(np.uint32) != S.view(np.uint32)).any(axis=-1).sum()} pixels"
    assert same_bits(st["even_sum"], E)


def build(rt, sc, kind):
    return rt.DeviceScene(sc, wide=True, device_bvh=True) if kind == "refit" else rt.DeviceScene(sc, device_bvh=True)


# ---- 1. the contract, in both modes
@pytest.mark.parametrize("kind", ["refit", "rebuild"])
def test_the_contract(gpu, sg, kind):
    rt, refit = gpu, kind == "refit"
    sc0, sc1 = keys_of(sg)
    key0, key1 = rt.geometry_arrays(sc0), rt.geometry_arrays(sc1)
    assert np.abs(key1["positions"] - key0["positions"]).max() > 3.0  # a tenth of the 40-unit room
    s0, s1 = sensors_of(rt, sg, sc0)
    dev, ref = build(rt, sc0, kind), build(rt, sc0, kind)
    acc = dev.accumulator(W, H, sensor=s0, shutter=dict(key0=sc0, key1=sc1, sensor1=s1, slices=4, block=3, refit=refit))
    assert not acc.shutter_info()["static_lights"]
    acc.render(5)
    assert acc.shutter_times()["slice_changes"] == len(R.runs(0, 5, 4, 3)) == 2
    acc.render(11)
    assert acc.shutter_times()["slice_changes"] == len(R.runs(5, 11, 4, 3)) == 5
    S, E = expected_sums(rt, ref, key0, key1, s0, s1, 16, 4, 3, refit)
    assert_state(acc, S, E, 16)
    # and the slices differ: the sums are not those of the static scene
    update_raw(rt, ref, key0, refit)
    plain = ref.accumulator(W, H, sensor=s0)
    plain.render(16)
    assert not same_bits(plain.read()["sum"], S)
    for d in (dev, ref):
        d.close()


# ---- 2. K = 1 is a plain accumulator on the blended static scene, for every layer
def test_one_slice_is_a_plain_accumulator_on_the_blended_scene(gpu, sg):
    rt = gpu
    sc0, sc1 = keys_of(sg)
    key0, key1 = rt.geometry_arrays(sc0), rt.geometry_arrays(sc1)
    cam0 = sc0.camera
    cam1 = dataclasses.replace(cam0, position=(np.asarray(cam0.position, dtype=F) + np.array([0.5, 0.0, 0.25], dtype=F)).astype(F))
    s0, s1 = rt.Sensor.thin_lens(cam0, 0.05, 6.0, seed=3), rt.Sensor.thin_lens(cam1, 0.1, 9.0, seed=4)
    n_mats = len(sc0.materials)
    layers = dict(features=True, ids="material", id_slots=3, light_groups=dict(material_group=[m % 2 for m in range(n_mats)], background=1, n_groups=2))
    t = R.slice_time(0, 1, 0.25, 0.75)
    dev, ref = build(rt, sc0, "refit"), build(rt, sc0, "refit")
    acc = dev.accumulator(W, H, sensor=s0, shutter=dict(key0=sc0, key1=sc1, sensor1=s1, open=0.25, close=0.75, slices=1, block=2, refit=True), **layers)
    acc.render(3)
    acc.render(4)
    assert acc.shutter_times()["slice_changes"] == 1  # K = 1: one run per call
    update_raw(rt, ref, R.geometry_at(key0, key1, t), True)
    plain = ref.accumulator(W, H, sensor=R.sensor_at(s0, s1, t), **layers)
    plain.render(7)
    for read in ("read", "read_features", "read_ids"):
        a, b = getattr(acc, read)(), getattr(plain, read)()
        for name in a:
            if name != "error":
                assert same_bits(a[name], b[name]), (read, name)
    assert same_bits(acc.read_light_groups(), plain.read_light_groups())
    for d in (dev, ref):
        d.close()


# ---- 3. equal keys and no second view: a plain accumulator after update_geometry(key 0)
@pytest.mark.parametrize("kind", ["refit", "rebuild"])
def test_equal_keys_are_a_plain_accumulator(gpu, sg, kind):
    rt, refit = gpu, kind == "refit"
    sc0 = room(sg)
    key0 = rt.geometry_arrays(sc0)
    dev, ref = build(rt, sc0, kind), build(rt, sc0, kind)
    acc = dev.accumulator(W, H, seed=7, shutter=dict(key0=sc0, key1=sc0, slices=4, block=1, refit=refit))
    assert acc.shutter_info()["static_lights"]
    acc.render(6)
    update_raw(rt, ref, key0, refit)
    plain = ref.accumulator(W, H, seed=7)
    plain.render(6)
    a, b = acc.read(), plain.read()
    assert same_bits(a["sum"], b["sum"]) and same_bits(a["even_sum"], b["even_sum"]) and (a["samples"] == 6).all()
    for d in (dev, ref):
        d.close()


# ---- 4. a camera-only shutter on scenes that cannot be updated in place: parity topology, analytic primitives
@pytest.mark.parametrize("which", ["parity", "txt"])
def test_camera_only_shutter(gpu, sg, which):
    rt = gpu
    if which == "parity":
        sc = room(sg)
        dev, cam0 = rt.DeviceScene(sc), sc.camera
    else:
        from conftest import SCENE000

        ls = rt.parse_scene_txt(SCENE000)
        assert ls.desc.n_primitives > 0  # analytic primitives: a scene rt_update_geometry has nothing to say about
        dev, cam0 = rt.DeviceScene(ls), ls.cameras()[0]
    cam1 = dataclasses.replace(cam0, position=(np.asarray(cam0.position, dtype=F) + np.array([0.25, 0.125, -0.25], dtype=F)).astype(F))
    s0, s1 = rt.Sensor.pinhole(cam0, seed=21), rt.Sensor.pinhole(cam1, seed=22)
    acc = dev.accumulator(W, H, sensor=s0, shutter=dict(sensor1=s1, slices=2, block=2))
    acc.render(3)
    acc.render(5)
    # render_sensors gives whole prefixes of a view's samples only, so the single samples of a slice come from sensor_rays + render_rays
    S, E = expected_sums(rt, dev, None, None, s0, s1, 8, 2, 2, False)
    assert_state(acc, S, E, 8)
    acc.close()
    # ... and where a slice is a prefix, from render_sensors itself: K = 1, the whole call at one time
    acc1 = dev.accumulator(W, H, sensor=s0, shutter=dict(sensor1=s1, slices=1, block=1))
    acc1.render(4)
    img, _ = dev.render_sensors(W, H, 4, [R.sensor_at(s0, s1, R.slice_time(0, 1))])
    assert same_bits(acc1.image(), img[0])
    dev.close()


# ---- 5. static lights: the light half of a refit slice is skipped, exactly
def test_static_lights_skip_the_light_rebuild(gpu, sg):
    rt = gpu
    sc0, sc1 = keys_of(sg, lights_move=False)
    key0, key1 = rt.geometry_arrays(sc0), rt.geometry_arrays(sc1)
    s0, s1 = sensors_of(rt, sg, sc0)
    dev, ref = build(rt, sc0, "refit"), build(rt, sc0, "refit")
    acc = dev.accumulator(W, H, sensor=s0, shutter=dict(key0=sc0, key1=sc1, sensor1=s1, slices=4, block=3, refit=True))
    assert acc.shutter_info() == {"static_lights": True, "light_rebuilds": 1}  # key 0 at attach
    acc.render(5)
    acc.render(11)
    assert acc.shutter_info() == {"static_lights": True, "light_rebuilds": 1}
    S, E = expected_sums(rt, ref, key0, key1, s0, s1, 16, 4, 3, True)  # every slice of `ref` rebuilds its light tree
    assert_state(acc, S, E, 16)
    acc.close()
    # one emitter, one float, one ulp: the rebuild path, still exact
    p = np.asarray(sc1.positions, dtype=F).copy()
    p[N_WALLS + 1, 2, 0] = np.nextafter(p[N_WALLS + 1, 2, 0], F(np.inf))
    sc2 = dataclasses.replace(sc1, positions=p)
    key2 = rt.geometry_arrays(sc2)
    acc = dev.accumulator(W, H, sensor=s0, shutter=dict(key0=sc0, key1=sc2, sensor1=s1, slices=4, block=3, refit=True))
    assert acc.shutter_info() == {"static_lights": False, "light_rebuilds": 1}
    acc.render(16)
    runs = len(R.runs(0, 16, 4, 3))
    assert acc.shutter_info()["light_rebuilds"] == 1 + runs + 1  # every slice and the return to key 0
    update_raw(rt, ref, key0, True)
    S, E = expected_sums(rt, ref, key0, key2, s0, s1, 16, 4, 3, True)
    assert_state(acc, S, E, 16)
    for d in (dev, ref):
        d.close()


# ---- 6. what a call leaves behind, and the refusals
def test_after_return_and_refusals(gpu, sg):
    rt = gpu
    INVALID, UNSUPPORTED = code(rt, "RT_ERR_INVALID_ARG"), code(rt, "RT_ERR_UNSUPPORTED")
    sc0, sc1 = keys_of(sg)
    key0 = rt.geometry_arrays(sc0)
    dev, ref = build(rt, sc0, "refit"), build(rt, sc0, "refit")
    update_raw(rt, ref, key0, True)
    want, _ = ref.run_raytracer(W, H, 4, seed=5)

    def unchanged():
        got, _ = dev.run_raytracer(W, H, 4, seed=5)
        return same_bits(got, want)

    def refused(call, err):
        with pytest.raises(rt.RtError) as e:
            call()
        assert e.value.code == err, str(e.value)
        assert unchanged()
        return str(e.value)

    acc = dev.accumulator(W, H, seed=2, shutter=dict(key0=sc0, key1=sc1, slices=4, block=2, refit=True))
    assert unchanged()  # after attach
    acc.render(5)
    assert unchanged()  # after a call that ended in the middle of a block
    before = acc.read()
    refused(lambda: dev.update_geometry(sc1, refit=True), INVALID)
    refused(lambda: dev.accumulator(W, H, seed=3), INVALID)
    refused(lambda: acc.render_adaptive(0.1, min_samples=2, max_samples=8), UNSUPPORTED)
    refused(lambda: acc.attach_shutter(key0=sc0, key1=sc1, slices=2, block=1), INVALID)  # a second attach, and after samples
    after = acc.read()
    assert same_bits(before["sum"], after["sum"]) and (after["samples"] == 5).all()
    acc.close()
    # refusals of attach leave the scene and the accumulator as they were
    plain = dev.accumulator(W, H, seed=2)
    for bad in (dict(slices=3), dict(slices=2048), dict(block=0), dict(open=0.5, close=0.25), dict(close=1.5), dict(open=float("nan")), dict(reserved=[0, 1])):
        refused(lambda bad=bad: plain.attach_shutter(**{**dict(key0=sc0, key1=sc1, slices=2, block=1), **bad}), INVALID)
    nan = np.asarray(sc1.positions, dtype=F).copy()
    nan[40, 1, 1] = np.nan
    assert "triangle 40" in refused(lambda: plain.attach_shutter(key0=sc0, key1=dataclasses.replace(sc1, positions=nan)), INVALID)
    bad_ids = np.full_like(sc0.material_ids, 1000)  # (the ids are key 0's)
    refused(lambda: plain.attach_shutter(key0=dataclasses.replace(sc0, material_ids=bad_ids), key1=dataclasses.replace(sc1, material_ids=bad_ids)), INVALID)
    short = dataclasses.replace(sc0, positions=sc0.positions[:-1], texcoords=sc0.texcoords[:-1], tangents=sc0.tangents[:-1], material_ids=sc0.material_ids[:-1])
    refused(lambda: plain.attach_shutter(key0=short, key1=short), INVALID)
    refused(lambda: plain.attach_shutter(sensor1=rt.Sensor.equirect(sc0.camera)), INVALID)  # another kind
    other = dev.accumulator(W, H, seed=9)
    refused(lambda: plain.attach_shutter(key0=sc0, key1=sc1), INVALID)  # another live accumulator
    other.close()
    plain.render(2)
    refused(lambda: plain.attach_shutter(key0=sc0, key1=sc1), INVALID)  # after samples
    twin = ref.accumulator(W, H, seed=2)
    twin.render(2)
    assert same_bits(plain.read()["sum"], twin.read()["sum"])
    plain.close()
    # REFIT needs a wide scene
    binary = build(rt, sc0, "rebuild")
    b = binary.accumulator(W, H, seed=2)
    with pytest.raises(rt.RtError) as e:
        b.attach_shutter(key0=sc0, key1=sc1, refit=True)
    assert e.value.code == UNSUPPORTED
    binary.close()
    # after close() the scene takes updates and accumulators again
    dev.update_geometry(sc1, refit=True)
    dev.accumulator(W, H, seed=3).close()
    for d in (dev, ref):
        d.close()


# ---- 7. a picture check that does not go through the replay's sums
def test_a_translating_quad_covers_each_pixel_in_the_slices_it_should(gpu, sg):
    rt = gpu
    PX = 0.25  # world units per pixel: an orthographic film 8 units wide over 32 pixels
    K, STEP, QW, ROWS = 8, 8, 16, (6, 18)  # the quad is 16 x 12 pixels and moves 8 pixels per slice
    left0 = -28  # pixels; at slice k its left edge is at left0 + (k + 0.5) * STEP = -24 + 8k

    def quad(left_px, z, rows, width_px):
        x0, x1 = -4.0 + PX * left_px, -4.0 + PX * (left_px + width_px)
        y0, y1 = 3.0 - PX * rows[1], 3.0 - PX * rows[0]
        a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
        return np.array([[a, b, c], [a, c, d]], dtype=F)

    def scene(left_px):
        pos = np.concatenate([quad(left_px, 0.0, ROWS, QW), quad(-400, -50.0, (-400, 400), 800)])
        tex = np.zeros((4, 3, 2), dtype=F)
        tan = np.zeros((4, 3, 3), dtype=F)
        tan[..., 0] = 1
        cam = sg.Camera(position=np.array([0, 0, 5], dtype=F), right=np.array([1, 0, 0], dtype=F), up=np.array([0, 1, 0], dtype=F),
                        forward=np.array([0, 0, -1], dtype=F), fov_x=1.0)
        mats = [sg.Material(color=(0.8, 0.2, 0.2, 1.0), roughness=1.0, metallic=0.0), sg.Material(color=(0.5, 0.5, 0.5, 1.0), roughness=1.0, metallic=0.0)]
        return sg.Scene(pos, None, tex, tan, np.array([0, 0, 1, 1], dtype=np.uint32), mats, camera=cam)

    sc0, sc1 = scene(left0), scene(left0 + K * STEP)
    dev = rt.DeviceScene(sc0, device_bvh=True)
    acc = dev.accumulator(W, H, sensor=rt.Sensor.orthographic(sc0.camera, half_width=4.0, seed=13), ids="primitive", id_slots=4,
                          shutter=dict(key0=sc0, key1=sc1, slices=K, block=1, refit=False))
    acc.render(K)
    ids = acc.read_ids()
    on_quad = np.where(ids["ids"] < 2, ids["counts"], 0).sum(axis=-1)
    assert (ids["counts"].sum(axis=-1) + ids["other"] == K).all()
    lefts = [left0 + STEP // 2 + STEP * k for k in range(K)]
    edges_x = sorted({e for left in lefts for e in (left, left + QW)})
    xs, ys = np.arange(W), np.arange(H)
    clear_x = np.array([all(x >= e + 1 or x + 1 <= e - 1 for e in edges_x) for x in xs])
    clear_y = np.array([all(y >= e + 1 or y + 1 <= e - 1 for e in ROWS) for y in ys])
    covered_x = np.array([sum(left <= x < left + QW for left in lefts) for x in xs])
    in_rows = (ys >= ROWS[0]) & (ys < ROWS[1])
    want = np.outer(in_rows, covered_x)
    interior = np.outer(clear_y, clear_x)
    swept = want > 0
    assert (interior & swept).sum() >= 0.5 * swept.sum() and swept.sum() == W * (ROWS[1] - ROWS[0])
    assert np.array_equal(on_quad[interior], want[interior])
    assert covered_x.max() == 2 and (on_quad[interior & swept] > 0).all() and (on_quad[interior & ~swept] == 0).all()
    dev.close()


# ---- 8. a wide scene small enough that its rebuild goes through the host collapse
@pytest.mark.parametrize("kind", ["refit", "rebuild"])
def test_the_contract_on_a_scene_of_eight_triangles(gpu, sg, kind):
    rt, refit = gpu, kind == "refit"
    big = room(sg)
    pick = np.r_[N_WALLS : N_WALLS + 2, 0:6]  # two lights and six wall triangles
    sc0 = dataclasses.replace(big, positions=big.positions[pick], texcoords=big.texcoords[pick], tangents=big.tangents[pick], material_ids=big.material_ids[pick])
    sc1 = moved(moved(sc0, slice(2, 5), (1.5, -1.0, 0.5)), slice(0, 1), (1.0, -0.25, 0.0))
    key0, key1 = rt.geometry_arrays(sc0), rt.geometry_arrays(sc1)
    s0, s1 = sensors_of(rt, sg, sc0)
    dev, ref = rt.DeviceScene(sc0, wide=True, device_bvh=True), rt.DeviceScene(sc0, wide=True, device_bvh=True)
    acc = dev.accumulator(W, H, sensor=s0, shutter=dict(key0=sc0, key1=sc1, sensor1=s1, slices=2, block=3, refit=refit))
    acc.render(4)
    acc.render(4)
    S, E = expected_sums(rt, ref, key0, key1, s0, s1, 8, 2, 3, refit)
    assert_state(acc, S, E, 8)
    for d in (dev, ref):
        d.close()


# ---- 9. keys that are in HBM already (RT_FLAG_DEVICE_FB): the same accumulator as from host keys, and the caller's tensors are not kept
def test_device_keys_equal_host_keys(gpu, sg):
    import torch

    rt = gpu
    sc0, sc1 = keys_of(sg)
    s0, s1 = sensors_of(rt, sg, sc0)
    devs = [build(rt, sc0, "refit"), build(rt, sc0, "refit")]
    kw = dict(sensor1=s1, slices=2, block=2, refit=True)
    host = devs[0].accumulator(W, H, sensor=s0, shutter=dict(key0=sc0, key1=sc1, **kw))
    tens = [{k: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0") for k, a in rt.geometry_arrays(sc).items()} for sc in (sc0, sc1)]
    ondev = devs[1].accumulator(W, H, sensor=s0, shutter=dict(key0=tens[0], key1=tens[1], **kw))
    for t in tens:  # copied at attach: the caller may overwrite theirs
        for v in t.values():
            v.zero_()
    torch.cuda.synchronize()
    for acc in (host, ondev):
        acc.render(6)
    a, b = host.read(), ondev.read()
    assert same_bits(a["sum"], b["sum"]) and same_bits(a["even_sum"], b["even_sum"]) and (b["samples"] == 6).all()
    with pytest.raises(rt.RtError) as e:  # a host pointer under the device flag is refused before anything is read
        bad = rt._ctypes_abi.RtShutterDesc()
        arrays = rt.geometry_arrays(sc0)
        bad.n_triangles, bad.mode, bad.slices, bad.block, bad.close, bad.flags = arrays["material_ids"].size, rt.RT_UPDATE_REFIT, 2, 1, 1.0, rt.RT_FLAG_DEVICE_FB
        for i in range(2):
            bad.positions[i], bad.normals[i], bad.tangents[i] = arrays["positions"].ctypes.data, arrays["normals"].ctypes.data, arrays["tangents"].ctypes.data
        bad.texcoords, bad.material_ids = arrays["texcoords"].ctypes.data, arrays["material_ids"].ctypes.data
        host.close()
        plain = devs[0].accumulator(W, H, seed=1)
        rt._check(rt.lib().rt_accum_attach_shutter(plain._h, C.byref(bad)))
    assert e.value.code == code(rt, "RT_ERR_INVALID_ARG") and "not device memory" in str(e.value)
    for d in devs:
        d.close()
