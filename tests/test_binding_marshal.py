"""The binding's shared marshalling rules (_marshal.py), without the library and without a GPU: a call's rt_params, where a result is
delivered, the device forms of the inputs, and the descriptors of the accumulator layers."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest

M = importlib.import_module("raytracing-course-hw-public_amd._marshal")
abi = importlib.import_module("raytracing-course-hw-public_amd._ctypes_abi")
sg = importlib.import_module("raytracing-course-hw-public_amd.scenegen")
DEVICE_FB = abi.RT_FLAG_DEVICE_FB


# ------------------------------------------------------------------------------------------------ rt_params
@pytest.mark.parametrize("counters, megakernel, global_best", list(itertools.product((False, True), repeat=3)))
def test_params_flags(counters, megakernel, global_best):
    p, keep = M._params(7, 5, 3, abi.RT_RNG_REFERENCE, 11, (1, 4, 2), counters, megakernel, global_best)
    assert p.flags == (abi.RT_FLAG_COUNTERS if counters else 0) | (abi.RT_FLAG_MEGAKERNEL if megakernel else 0) | (abi.RT_FLAG_GLOBAL_BEST if global_best else 0)
    assert (p.width, p.height, p.samples, p.rng_mode, p.seed) == (7, 5, 3, abi.RT_RNG_REFERENCE, 11)
    assert (p.shard_index, p.shard_count, p.shard_block) == (1, 4, 2) and keep is None


def test_params_defaults_and_tuning():
    p, keep = M._params(2, 2, 1)
    assert (p.rng_mode, p.seed, p.shard_index, p.shard_count, p.shard_block, p.flags) == (abi.RT_RNG_DEVICE, 0, 0, 1, 0, 0)
    assert (p.sort_mode, p.packet_mode, p.packet_min_lanes, p.max_paths) == (0, 0, 0.0, 0) and not p.progress and keep is None
    p, keep = M._params(2, 2, 1, tuning=dict(sort_mode=np.int64(6), packet_mode=2, packet_min_lanes=12, max_paths=1 << 33, progress=None))
    assert (p.sort_mode, p.packet_mode, p.max_paths) == (6, 2, 1 << 33) and p.packet_min_lanes == 12.0 and not p.progress and keep is None
    with pytest.raises(TypeError):
        M._params(2, 2, 1, tuning=dict(sort_mod=1))
    seen = []
    p, keep = M._params(2, 2, 1, tuning=dict(progress=lambda done, total: seen.append((done, total))))
    assert isinstance(keep, abi.RT_PROGRESS_FN) and p.progress
    p.progress(3, 9, None)  # as the library calls it: (done, total, user)
    assert seen == [(3, 9)]


# ------------------------------------------------------------------------------------------------ delivery
class FakeCall:
    def __init__(self):
        self.calls = []

    def __call__(self, flags, *pointers):
        self.calls.append((flags, [ctypes.cast(p, ctypes.c_void_p).value for p in pointers]))
        return abi.RT_OK


def test_deliver_host_and_device_forms():
    call = FakeCall()
    out = M._deliver(call, (3, 5, 2), np.uint8)
    assert out.shape == (3, 5, 2) and out.dtype == np.uint8 and not out.any() and call.calls == [(0, [out.ctypes.data])]
    rays = M._deliver(call, (6,), abi.RAY_DTYPE)
    assert rays.shape == (6,) and rays.dtype == abi.RAY_DTYPE and call.calls[-1] == (0, [rays.ctypes.data])
    assert M._deliver(call, (3, 5, 2), np.uint8, device=0x7000) is None and call.calls[-1] == (DEVICE_FB, [0x7000])
    mine = np.ones((4, 2, 3), dtype=np.float32)
    assert M._deliver(call, (4, 2, 3), np.float32, out=mine) is mine and call.calls[-1] == (0, [mine.ctypes.data]) and mine.all()
    assert M._deliver(call, (4, 2, 3), np.float32, device=0x7000, out=mine) is None  # the device form wins, as it always has
    n = len(call.calls)
    for bad in (np.ones((4, 2, 3), dtype=np.float64), np.ones((4, 2, 2), dtype=np.float32), np.ones((4, 2, 6), dtype=np.float32)[:, :, ::2]):
        with pytest.raises(AssertionError):
            M._deliver(call, (4, 2, 3), np.float32, out=bad)
    assert len(call.calls) == n


def test_deliver_each_and_render():
    call = FakeCall()
    out = M._deliver_each(call, (2, 3), dict(flow=(np.float32, 2), valid=(np.uint32,)))
    assert list(out) == ["flow", "valid"] and out["flow"].shape == (2, 3, 2) and out["flow"].dtype == np.float32
    assert out["valid"].shape == (2, 3) and out["valid"].dtype == np.uint32 and call.calls == [(0, [out["flow"].ctypes.data, out["valid"].ctypes.data])]
    assert M._deliver_each(call, (2, 3), dict(a=(np.float32,), b=(np.float32,)), device=(0x100, None)) == {"a": None, "b": None}
    assert call.calls[-1] == (DEVICE_FB, [0x100, None])
    with pytest.raises(ValueError):
        M._deliver_each(call, (2, 3), dict(a=(np.float32,), b=(np.float32,)), device=(1, 2, 3))
    seen = []

    def fn(handle, params, middle, pointer, stats):
        seen.append((handle, ctypes.cast(params, ctypes.POINTER(abi.RtParams)).contents.flags, middle))
        ctypes.cast(stats, ctypes.POINTER(abi.RtStats)).contents.samples = 12
        return abi.RT_OK

    p, _ = M._params(3, 2, 1, global_best=True)
    img, st = M._render(fn, 77, p, ("mid",), (2, 3, 3), np.float32)
    assert img.shape == (2, 3, 3) and st["samples"] == 12 and seen == [(77, abi.RT_FLAG_GLOBAL_BEST, "mid")]
    img, st = M._render(fn, 77, p, ("mid",), (2, 3, 3), np.float32, device=0x500)
    assert img is None and seen[-1] == (77, abi.RT_FLAG_GLOBAL_BEST | DEVICE_FB, "mid")


def test_paired_device_buffers():
    assert M._device_pair("bake", "points", None, None, None) is False and M._device_pair("bake", "points", 0, 5, 0) is False
    assert M._device_pair("bake", "points", 0x10, 5, 0x20) is True
    for device_in, count, device_out in ((0x10, 5, None), (None, 5, 0x20), (0x10, None, 0x20)):
        with pytest.raises(ValueError):
            M._device_pair("render_rays", "rays", device_in, count, device_out)


# ------------------------------------------------------------------------------------------------ device arrays
def test_device_array_check():
    import torch

    assert M._device_array("positions", 0x1000, 9, n=4) == (0x1000, 4, None)
    rows = [("positions", 0x1000, 9, ("float32",)), ("normals", 0x2000, 9, ("float32",))]
    assert M._device_arrays(rows, 4) == ([0x1000, 0x2000], 4)
    with pytest.raises(ValueError):
        M._device_arrays(rows)  # every array is a pointer: nothing says how many triangles
    with pytest.raises(TypeError):
        M._device_array("positions", torch.zeros(18), 9)  # on the CPU
    with pytest.raises(TypeError):
        M._device_array("positions", np.zeros(18, dtype=np.float32), 9)
    with pytest.raises(TypeError):
        M._device_array("positions", 0x1000, 9, pointer_ok=False)
    with pytest.raises(TypeError):
        M._device_array("positions", True, 9)


# ------------------------------------------------------------------------------------------------ descriptors
def _key(shift):
    """A two-triangle key as a scenegen.Scene."""
    rng = np.random.default_rng(5)
    pos = rng.uniform(-1, 1, size=(2, 3, 3)).astype(np.float32) + np.float32(shift)
    zero = np.zeros(3, dtype=np.float32)
    return sg.Scene(positions=pos, normals=None, texcoords=rng.uniform(0, 1, size=(2, 3, 2)).astype(np.float32), tangents=np.ones((2, 3, 3), dtype=np.float32),
                    material_ids=np.array([0, 1], dtype=np.uint32), materials=[], camera=sg.Camera(zero, zero, zero, zero, 1.0))


def _arrays(scene):
    return dict(positions=scene.positions, normals=scene.resolved_normals(), texcoords=scene.texcoords, tangents=scene.tangents, material_ids=scene.material_ids)


def _sensor1():
    e = np.eye(3, dtype=np.float32)
    rt = importlib.import_module("raytracing-course-hw-public_amd")
    return rt.Sensor.pinhole(sg.Camera(np.array([1, 2, 3], dtype=np.float32), e[0], e[1], e[2], 0.9), seed=4)


def _addr(pointer):
    return ctypes.cast(pointer, ctypes.c_void_p).value


@pytest.mark.parametrize("form", ["scene", "arrays"])
def test_shutter_descriptor_from_host_keys(form):
    k0, k1 = _key(0.0), _key(0.25)
    keys = (k0, k1) if form == "scene" else (_arrays(k0), _arrays(k1))
    d, keep = M._shutter_desc(*keys, _sensor1(), 0.125, 0.75, 8, 2, False, None)
    assert (d.n_triangles, d.flags, d.mode, d.open, d.close, d.slices, d.block) == (2, 0, abi.RT_UPDATE_REBUILD, 0.125, 0.75, 8, 2)
    a0, a1, rec = keep
    for i, a in enumerate((a0, a1)):
        assert (d.positions[i], d.normals[i], d.tangents[i]) == (a["positions"].ctypes.data, a["normals"].ctypes.data, a["tangents"].ctypes.data)
        assert np.array_equal(a["positions"], keys[i]["positions"].reshape(-1) if form == "arrays" else keys[i].positions.reshape(-1))
    assert (d.texcoords, d.material_ids) == (a0["texcoords"].ctypes.data, a0["material_ids"].ctypes.data)
    assert _addr(d.sensor1) == ctypes.addressof(rec) and d.sensor1.contents.seed == 4 and list(d.sensor1.contents.camera.position) == [1, 2, 3]
    assert list(d.reserved) == [0] * 7
    d, keep = M._shutter_desc(k0, k1, None, 0.0, 1.0, 16, 4, True, (0, 0, 3))
    assert d.mode == abi.RT_UPDATE_REFIT and not d.sensor1 and len(keep) == 2 and list(d.reserved) == [0, 0, 3, 0, 0, 0, 0]


@pytest.mark.parametrize("form", ["scene", "arrays", "ndarray"])
def test_flow_descriptor_from_host_keys(form):
    k0, k1 = _key(0.0), _key(0.25)
    keys = {"scene": (k0, k1), "arrays": (_arrays(k0), _arrays(k1)), "ndarray": (k0.positions, k1.positions)}[form]
    d, keep = M._flow_desc(*keys, _sensor1(), None)
    a0, a1, rec = keep
    assert (d.n_triangles, d.flags) == (2, 0) and (d.positions[0], d.positions[1]) == (a0["positions"].ctypes.data, a1["positions"].ctypes.data)
    assert np.array_equal(a0["positions"], k0.positions.reshape(-1)) and np.array_equal(a1["positions"], k1.positions.reshape(-1))
    assert _addr(d.sensor1) == ctypes.addressof(rec) and list(d.reserved) == [0] * 8
    d, keep = M._flow_desc(*keys, None, (5,))
    assert not d.sensor1 and len(keep) == 2 and list(d.reserved) == [5, 0, 0, 0, 0, 0, 0, 0]


def test_descriptors_without_keys():
    d, keep = M._shutter_desc(None, None, _sensor1(), 0.0, 1.0, 16, 4, True, None)
    assert (d.n_triangles, d.flags) == (0, 0) and len(keep) == 1 and d.sensor1
    assert [d.positions[0], d.positions[1], d.normals[0], d.normals[1], d.tangents[0], d.tangents[1], d.texcoords, d.material_ids] == [None] * 8
    d, keep = M._flow_desc(None, None, None, None)
    assert (d.n_triangles, d.flags, d.positions[0], d.positions[1]) == (0, 0, None, None) and not d.sensor1 and keep == []


@pytest.mark.parametrize("build", [lambda a, b: M._shutter_desc(a, b, None, 0.0, 1.0, 16, 4, True, None), lambda a, b: M._flow_desc(a, b, None, None)], ids=["shutter", "flow"])
def test_descriptor_key_refusals(build):
    import torch

    k0, k1 = _key(0.0), _key(0.25)
    three = sg.Scene(positions=np.random.default_rng(1).uniform(size=(3, 3, 3)).astype(np.float32), normals=None, texcoords=np.zeros((3, 3, 2), dtype=np.float32),
                     tangents=np.ones((3, 3, 3), dtype=np.float32), material_ids=np.zeros(3, dtype=np.uint32), materials=[], camera=k0.camera)
    cpu = {name: torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)) for name, a in _arrays(k0).items()}
    for a, b in ((k0, None), (None, k1), (k0, three)):
        with pytest.raises(ValueError):
            build(a, b)
    with pytest.raises(ValueError):
        build(k0, cpu)  # one key on the host, the other a tensor key
    with pytest.raises(TypeError):
        build(cpu, dict(cpu))  # tensor keys, but not CUDA tensors


def test_flow_refuses_bare_cpu_tensors():
    import torch

    t = torch.zeros(18)
    with pytest.raises(ValueError):
        M._flow_desc(np.zeros((2, 3, 3), dtype=np.float32), t, None, None)
    with pytest.raises(TypeError):
        M._flow_desc(t, t.clone(), None, None)


def test_ids_descriptor():
    d, keep = M._ids_desc("primitive", 4, None)
    assert (d.kind, d.slots, d.table, d.n_table, d.flags) == (abi.RT_ID_PRIMITIVE, 4, None, 0, 0) and keep == []
    assert M._ids_desc("material", 0, None)[0].kind == abi.RT_ID_MATERIAL
    d, keep = M._ids_desc([7, 7, 9], 2, None)
    assert (d.kind, d.slots, d.table, d.n_table, d.flags) == (abi.RT_ID_USER, 2, keep[0].ctypes.data, 3, 0) and keep[0].dtype == np.uint32 and list(keep[0]) == [7, 7, 9]
    d, keep = M._ids_desc(0x9000, 4, 12)
    assert (d.kind, d.table, d.n_table, d.flags) == (abi.RT_ID_USER, 0x9000, 12, DEVICE_FB) and keep == []
    for bad in ("triangle", 0x9000):
        with pytest.raises(ValueError):
            M._ids_desc(bad, 4, None)


def test_light_groups_descriptor():
    none = abi.RT_LIGHT_GROUP_NONE
    d, keep = M._light_groups_desc([0, None, 2, 1], None, None, None)
    assert (d.n_groups, d.background_group, d.material_group, d.n_materials, d.flags) == (3, none, keep[0].ctypes.data, 4, 0) and list(keep[0]) == [0, none, 2, 1]
    assert M._light_groups_desc([0, None], 4, None, None)[0].n_groups == 5 and M._light_groups_desc([0, None], 4, None, None)[0].background_group == 4
    assert M._light_groups_desc([None, None], None, None, None)[0].n_groups == 1 and M._light_groups_desc([0, 1], None, 6, None)[0].n_groups == 6
    d, keep = M._light_groups_desc(0x9000, 1, 2, 7)
    assert (d.n_groups, d.background_group, d.material_group, d.n_materials, d.flags) == (2, 1, 0x9000, 7, DEVICE_FB) and keep == []
    for n_groups, n_materials in ((None, 7), (2, None)):
        with pytest.raises(ValueError):
            M._light_groups_desc(0x9000, None, n_groups, n_materials)


def test_denoise_descriptor():
    d, _ = M._denoise_desc({})
    assert bytes(d) == bytes(ctypes.sizeof(abi.RtDenoise))  # all-zero: the defaults
    d, _ = M._denoise_desc(dict(demodulate=False, iterations=3, sigma_color=0.5, sigma_depth=2, normal_sharpness=64, reserved=(0, 1)))
    assert (d.iterations, d.sigma_color, d.sigma_depth, d.normal_sharpness, d.flags, list(d.reserved)) == (3, 0.5, 2.0, 64, abi.RT_DENOISE_NO_DEMODULATE, [0, 1, 0])
    assert M._denoise_desc(dict(demodulate=True))[0].flags == 0 and M._denoise_desc(dict(demodulate=False, flags=4))[0].flags == 4 | abi.RT_DENOISE_NO_DEMODULATE
    with pytest.raises(TypeError):
        M._denoise_desc(dict(sigma=1.0))
