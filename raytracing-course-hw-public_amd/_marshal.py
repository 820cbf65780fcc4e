"""The marshalling rules every entry point of the binding shares, each stated once: a call's rt_params, where a result is delivered, the
device forms of the inputs, and the descriptors of the accumulator layers. Nothing here calls the library except through the closures it
is handed, so all of it is tested without a GPU (tests/test_binding_marshal.py)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._ctypes_abi import (RT_DENOISE_NO_DEMODULATE, RT_FLAG_COUNTERS, RT_FLAG_DEVICE_FB, RT_FLAG_GLOBAL_BEST, RT_FLAG_MEGAKERNEL, RT_ID_MATERIAL,
                          RT_ID_PRIMITIVE, RT_ID_USER, RT_LIGHT_GROUP_NONE, RT_PROGRESS_FN, RT_RNG_DEVICE, RT_UPDATE_REBUILD, RT_UPDATE_REFIT, RtDenoise,
                          RtFlowDesc, RtIdDesc, RtLightGroupDesc, RtParams, RtSensor, RtShutterDesc, RtStats)
from ._library import _check
from ._records import GEOMETRY_ARRAYS, geometry_arrays
from ._sensors import make_sensors


def _apply_tuning(p: RtParams, tuning: dict):
    """rt_params' ABI-4 fields from keyword arguments; returns the ctypes callback object (if any), to be kept alive by the caller."""
    cb = None
    for k, v in tuning.items():
        if k == "progress":
            if v is not None:
                cb = RT_PROGRESS_FN(lambda done, total, user, f=v: f(done, total))
                p.progress = cb
        elif k in ("sort_mode", "packet_mode", "max_paths"):
            setattr(p, k, int(v))
        elif k == "packet_min_lanes":
            p.packet_min_lanes = float(v)
        else:
            raise TypeError(f"rt_params has no tuning field {k!r}")
    return cb


def _params(width, height, samples, rng_mode=RT_RNG_DEVICE, seed=0, shard=(0, 1, 0), counters=False, megakernel=False, global_best=False, tuning=None):
    """One call's rt_params: `shard` is (shard_index, shard_count, shard_block), `tuning` the entry point's **tuning. Returns (record, the
    object that keeps a progress callback alive: hold it until the call has returned)."""
    flags = (RT_FLAG_COUNTERS if counters else 0) | (RT_FLAG_MEGAKERNEL if megakernel else 0) | (RT_FLAG_GLOBAL_BEST if global_best else 0)
    p = RtParams(width, height, samples, rng_mode, seed, *shard, flags)
    return p, _apply_tuning(p, tuning or {})


def _deliver(call, shape, dtype, device=None, out=None):
    """Where the one output of call(flags, pointer) goes. `device` (a device pointer): there, with RT_FLAG_DEVICE_FB, and None is returned.
    Otherwise into a new zeroed array of `shape` (a tuple) and `dtype`, or into the caller's `out` (that dtype, contiguous, as many elements),
    which is returned."""
    if device:
        _check(call(RT_FLAG_DEVICE_FB, C.c_void_p(device)))
        return None
    if out is None:
        out = np.zeros(shape, dtype=dtype)
    else:
        assert out.dtype == dtype and out.flags["C_CONTIGUOUS"] and out.size == math.prod(shape)
    _check(call(0, out.ctypes.data_as(C.c_void_p)))
    return out


def _deliver_each(call, head, arrays, device=None):
    """_deliver for call(flags, *pointers) with one output per entry of `arrays` (name -> (dtype, *tail)), in that order: name -> a new zeroed
    array of shape head + tail. `device` (one device pointer per output; None or 0 for an output that is not wanted): there, with
    RT_FLAG_DEVICE_FB, and every value is None."""
    if device is not None:
        ptrs = dict(zip(arrays, device, strict=True))
        _check(call(RT_FLAG_DEVICE_FB, *[C.c_void_p(q or None) for q in ptrs.values()]))
        return dict.fromkeys(arrays)
    out = {name: np.zeros(tuple(head) + tuple(tail), dtype=dtype) for name, (dtype, *tail) in arrays.items()}
    _check(call(0, *[a.ctypes.data_as(C.POINTER(C.c_float if a.dtype == np.float32 else C.c_uint32)) for a in out.values()]))
    return out


def _render(fn, handle, p, middle, shape, dtype, device=None, out=None):
    """fn(handle, &p, *middle, pointer, &stats) of the render entry points, delivered as _deliver states with the flag in p.flags. Returns
    (the output or None, stats dict)."""
    st = RtStats()

    def call(flags, pointer):
        p.flags |= flags
        return fn(handle, C.byref(p), *middle, pointer, C.byref(st))

    return _deliver(call, shape, dtype, device, out), st.as_dict()


def _device_pair(who, what, device_in, count, device_out) -> bool:
    """The device form of a call with an input and an output buffer: device_<what> and device_out go together, and device_<what> needs
    n_<what>. True for the device form."""
    if bool(device_in) != bool(device_out):
        raise ValueError(f"{who}: device_{what} and device_out go together (RT_FLAG_DEVICE_FB covers both buffers)")
    if device_in and count is None:
        raise ValueError(f"{who}: device_{what} needs n_{what}")
    return bool(device_in)


def _device_array(name, a, per, dtypes=("float32",), n=None, pointer_ok=True, exact=True, strict=False, peer=None, scene_device=None):
    """One per-triangle array (`per` elements each) that is in HBM already: an int device pointer (`pointer_ok`), taken on trust, or a
    contiguous torch CUDA tensor of one of `dtypes` (torch dtype names; None: any 4-byte elements). `n`: the triangle count it must hold
    (None: its own, numel // per); `exact=False` does not compare and ignores a remainder. `strict`: a non-contiguous tensor is a
    ValueError of its own and numel must be a multiple of `per`. `peer` (a torch device) / `scene_device` (an ordinal): where it must be.
    The tensor's current stream is synchronised: the idle precondition. Returns (pointer, n, the tensor's device or None)."""
    if pointer_ok and isinstance(a, int) and not isinstance(a, bool):
        return a, n, None
    import torch

    want = "4-byte" if dtypes is None else " or ".join(dtypes)
    what = f"{name}: a contiguous {want} torch CUDA tensor" + (" or an int device pointer" if pointer_ok else "")
    if not isinstance(a, torch.Tensor) or not a.is_cuda:
        raise TypeError(f"{what}, not {type(a).__name__}" + (" on the CPU" if isinstance(a, torch.Tensor) else ""))
    if (a.element_size() != 4) if dtypes is None else (a.dtype not in [getattr(torch, t) for t in dtypes if hasattr(torch, t)]):
        raise TypeError(f"{what}, not dtype {a.dtype}")
    if not a.is_contiguous():
        raise (ValueError if strict else TypeError)(f"{what}: the tensor is not contiguous")
    if strict and a.numel() % per:
        raise ValueError(f"{name}: {a.numel()} elements are no multiple of {per} per triangle")
    if n is None or not exact:
        n = a.numel() // per
    if exact and a.numel() != n * per:
        raise ValueError(f"{name}: {a.numel()} elements, expected {n * per} for {n} triangles")
    if peer is not None and a.device != peer:
        raise ValueError(f"{name}: on {a.device}, the other arrays are on {peer}")
    if scene_device is not None and a.device.index != scene_device:
        raise ValueError(f"{name}: on {a.device}, the scene is on GPU {scene_device}")
    torch.cuda.current_stream(a.device).synchronize()
    return (a.data_ptr() if a.numel() else 0), n, a.device


def _device_arrays(arrays, n=None, same_device=False, **checks):
    """_device_array over (name, array, per, dtypes) rows that share one triangle count: `n_triangles`, or the first tensor's. Returns
    ([pointers], n)."""
    ptrs, device = [], None
    for name, a, per, dtypes in arrays:
        ptr, n, dev = _device_array(name, a, per, dtypes, n, peer=device if same_device else None, **checks)
        device = dev if device is None else device
        ptrs.append(ptr)
    if n is None:
        raise ValueError("n_triangles is needed when every array is a device pointer")
    return ptrs, n


def _geometry_keys(who, key0, key1, sensor1, rows):
    """The two geometry keys and the second view of a shutter or a flow layer. A key carries the arrays of `rows` ((name, per, torch dtype
    names) each): a scenegen.Scene, a LoadedScene or an arrays dict (read through geometry_arrays), a dict of torch CUDA tensors, or, where
    the key carries one array, that array or tensor itself. Both keys or neither; both on the host or both on the device; one triangle
    count. Returns ({name: (pointer of key 0, of key 1)} ({} without keys), n_triangles, the descriptor's flags, rt_sensor* of `sensor1` or
    None, [what the pointers need alive])."""
    keep, ptrs, n, on_device = [], {}, 0, None
    if (key0 is None) != (key1 is None):
        raise ValueError(f"{who}: give both geometry keys or neither")
    if key0 is not None:
        per_key, counts = [], set()
        for key in (key0, key1):
            bare = len(rows) == 1 and not isinstance(key, dict) and (hasattr(key, "data_ptr") or isinstance(key, np.ndarray))
            if bare:
                key = {rows[0][0]: key}
            dev_key = isinstance(key, dict) and any(hasattr(key.get(name), "data_ptr") for name, _, _ in rows)
            if on_device is not None and dev_key != on_device:
                raise ValueError(f"{who}: one key is on the device and the other is not")
            on_device = dev_key
            if dev_key:
                got = {name: _device_array(f"{who}: {name}", key[name], per, dtypes, pointer_ok=False, exact=False)[:2] for name, per, dtypes in rows}
            else:
                host = {name: np.ascontiguousarray(key[name], dtype=np.float32).reshape(-1) for name, _, _ in rows} if bare else geometry_arrays(key)
                keep.append(host)
                got = {name: (host[name].ctypes.data if host[name].size else 0, host[name].size // per) for name, per, _ in rows}
            per_key.append(got)
            counts |= {count for _, count in got.values()}
        if len(counts) != 1:
            raise ValueError(f"{who}: the arrays of the keys hold different triangle counts {sorted(counts)}")
        n = counts.pop()
        ptrs = {name: (per_key[0][name][0], per_key[1][name][0]) for name, _, _ in rows}
    sensor = None
    if sensor1 is not None:
        rec = make_sensors([sensor1])
        keep.append(rec)
        sensor = C.cast(rec, C.POINTER(RtSensor))
    return ptrs, n, RT_FLAG_DEVICE_FB if on_device else 0, sensor, keep


# ---- descriptors of the accumulator layers: (ctypes record, [what its pointers need alive]) of the Python arguments, no library call ----


def _reserved(d, reserved):
    for i, r in enumerate(reserved or ()):
        d.reserved[i] = int(r)


def _shutter_desc(key0, key1, sensor1, open, close, slices, block, refit, reserved):
    d = RtShutterDesc()
    d.mode = RT_UPDATE_REFIT if refit else RT_UPDATE_REBUILD
    d.open, d.close, d.slices, d.block = float(open), float(close), int(slices), int(block)
    _reserved(d, reserved)
    rows = [(name, per, ("float32",) if dtype == np.float32 else None) for name, per, dtype in GEOMETRY_ARRAYS]
    ptrs, d.n_triangles, d.flags, d.sensor1, keep = _geometry_keys("attach_shutter", key0, key1, sensor1, rows)
    if ptrs:
        for i in range(2):
            d.positions[i], d.normals[i], d.tangents[i] = ptrs["positions"][i], ptrs["normals"][i], ptrs["tangents"][i]
        d.texcoords, d.material_ids = ptrs["texcoords"][0], ptrs["material_ids"][0]  # key 0's
    return d, keep


def _flow_desc(key0, key1, sensor1, reserved):
    d = RtFlowDesc()
    _reserved(d, reserved)
    ptrs, d.n_triangles, d.flags, d.sensor1, keep = _geometry_keys("attach_flow", key0, key1, sensor1, [("positions", 9, ("float32",))])
    if ptrs:
        d.positions[0], d.positions[1] = ptrs["positions"]
    return d, keep


def _ids_desc(kind, slots, n_table):
    d, keep = RtIdDesc(), []
    d.slots = int(slots)
    if isinstance(kind, str):
        if kind not in ("primitive", "material"):
            raise ValueError(f"attach_ids: kind {kind!r} is not 'primitive', 'material', an array or a device pointer")
        d.kind = RT_ID_PRIMITIVE if kind == "primitive" else RT_ID_MATERIAL
    elif isinstance(kind, (int, np.integer)):
        if n_table is None:
            raise ValueError("attach_ids: a device pointer needs n_table")
        d.kind, d.table, d.n_table, d.flags = RT_ID_USER, int(kind), int(n_table), RT_FLAG_DEVICE_FB
    else:
        table = np.ascontiguousarray(kind, dtype=np.uint32).reshape(-1)
        keep.append(table)
        d.kind, d.table, d.n_table = RT_ID_USER, table.ctypes.data, table.size
    return d, keep


def _light_groups_desc(material_group, background, n_groups, n_materials):
    d, keep, none = RtLightGroupDesc(), [], RT_LIGHT_GROUP_NONE
    d.background_group = none if background is None else int(background)
    named = [] if background is None else [int(background)]
    if isinstance(material_group, (int, np.integer)):
        if n_materials is None or n_groups is None:
            raise ValueError("attach_light_groups: a device pointer needs n_materials and n_groups")
        d.material_group, d.n_materials, d.flags = int(material_group), int(n_materials), RT_FLAG_DEVICE_FB
    else:
        table = np.array([none if g is None else int(g) for g in material_group], dtype=np.uint32)
        keep.append(table)
        d.material_group, d.n_materials = table.ctypes.data, table.size
        named += [int(g) for g in table if g != none]
    d.n_groups = int(n_groups) if n_groups is not None else max(named, default=0) + 1
    return d, keep


def _denoise_desc(opts):
    d = RtDenoise()
    for k, v in opts.items():
        if k == "demodulate":
            if not v:
                d.flags |= RT_DENOISE_NO_DEMODULATE
        elif k == "reserved":
            _reserved(d, v)
        elif k in ("sigma_color", "sigma_depth"):
            setattr(d, k, float(v))
        elif k in ("iterations", "normal_sharpness", "flags"):
            setattr(d, k, int(v) | (d.flags if k == "flags" else 0))
        else:
            raise TypeError(f"rt_denoise has no field {k!r}")
    return d, []
