"""MI355X-native render loop for firelion9/raytracing-course-hw-public — Python host binding.

The product is the C-ABI shared library `csrc/librt_amd.so` (include/rt_abi.h + include/rt_host.h): hand-written
HIP kernels for gfx950 behind the seam the reference enters at `run_raytracer(scene, image)`
(src/raytracer.h:629). This module is a thin ctypes mirror of that ABI for tests and bench.py; names follow
the reference (`run_raytracer`, `parse_gltf_scene`, `Image.write`).

There is NO CPU fallback: if the library is missing, or no GPU is present when a device entry point is called,
the call raises.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
from typing import Optional, Tuple

import numpy as np

from . import rays  # noqa: F401
from . import scenegen  # noqa: F401
from ._ctypes_abi import (
    ABI_PROTOTYPES,
    ERROR_NAMES,
    HOST_PROTOTYPES,
    RT_ACCUM_FEATURES,
    RT_DENOISE_NO_DEMODULATE,
    RT_ID_PRIMITIVE,
    RT_ID_MATERIAL,
    RT_ID_USER,
    RT_ID_MISS,
    RT_ID_MAX_SLOTS,
    RT_LIGHT_GROUP_MAX,
    RT_LIGHT_GROUP_NONE,
    RT_FLAG_COUNTERS,
    RT_FLAG_DEVICE_FB,
    RT_BUILD_DEVICE_LBVH,
    RT_BUILD_WIDE,
    RT_BUILD_WIDE_HOST_COLLAPSE,
    RT_BUILD_GROUP_COPY,
    RT_BUILD_GROUP_SELF_EXCHANGE,
    RT_BUILD_TEX_TILED,
    RT_BUILDER_PLOC,
    RT_BUILDER_LBVH,
    RT_SORT_AUTO,
    RT_SORT_OFF,
    RT_SORT_OCTANT_CELL_CONE,
    RT_PACKET_AUTO,
    RT_PACKET_OFF,
    RT_PACKET_ON,
    RT_PROGRESS_FN,
    RT_FLAG_MEGAKERNEL,
    RT_FLAG_GLOBAL_BEST,
    RT_CAST_PROBE,
    RT_CAST_EXTEND,
    RT_CAST_EXTEND_GLOBAL,
    RT_CAST_PACKET,
    RT_CAST_PACKET_GLOBAL,
    RT_OK,
    RT_UPDATE_REBUILD,
    RT_UPDATE_REFIT,
    RT_ENV_IMPORTANCE,
    RT_FLOW_MEAN,
    RT_FLOW_NEAREST,
    RT_RNG_DEVICE,
    RT_RNG_REFERENCE,
    RAY_DTYPE,
    BAKE_POINT_DTYPE,
    RT_BAKE_IRRADIANCE,
    RT_BAKE_SH9,
    DescHolder,
    RtAdaptive,
    RtBake,
    RtBakePoint,
    RtCamera,
    RtDenoise,
    RtEnvironment,
    RtFlowDesc,
    RtGeometryUpdate,
    RtIdDesc,
    RtLightGroupDesc,
    RtParams,
    RtRay,
    RtSceneDesc,
    RtSensor,
    RtShutterDesc,
    RtView,
    RtStats,
    bind,
    c_float_p,
    c_u8_p,
    desc_to_arrays,
    fptr,
    u8ptr,
    u32ptr,
)

RT_ALL_DEVICES = -1
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT_AMD_LIB") or os.path.join(_HERE, "csrc", "librt_amd.so")  # RT_AMD_LIB: tuning variants only
_lib: Optional[C.CDLL] = None


class RtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERROR_NAMES.get(code, code)}: {msg}")
        self.code = code


def lib() -> C.CDLL:
    """Load csrc/librt_amd.so. Raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: the HIP library is not built; there is no CPU fallback. Run __graft_entry__.build().")
        _lib = C.CDLL(LIB_PATH)
        bind(_lib, ABI_PROTOTYPES)
        bind(_lib, HOST_PROTOTYPES)
    return _lib


def _check(code: int) -> None:
    if code != RT_OK:
        raise RtError(code, lib().rt_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    return int(lib().rt_device_count())


def write_flo(path, flow) -> None:
    """An (H, W, 2) flow field (Accumulator.flow) as a Middlebury .flo file: the float32 tag 202021.25 ("PIEH"), width and height as
    little-endian int32, then the (dx, dy) float32 pairs row by row."""
    f = np.asarray(flow, dtype="<f4")
    if f.ndim != 3 or f.shape[2] != 2:
        raise ValueError(f"write_flo: the flow must have shape (H, W, 2), not {f.shape}")
    with open(path, "wb") as out:
        out.write(np.array([202021.25], dtype="<f4").tobytes())
        out.write(np.array([f.shape[1], f.shape[0]], dtype="<i4").tobytes())
        out.write(np.ascontiguousarray(f).tobytes())


class LoadedScene:
    """Result of parse_gltf_scene (scene.h:183) through the C++ host loader; owns the C-side arrays."""

    def __init__(self, handle: C.c_void_p):
        self._h = handle
        self.desc: RtSceneDesc = lib().rt_loaded_desc(handle).contents

    def arrays(self) -> dict:
        return desc_to_arrays(self.desc)

    def info(self) -> dict:
        """DIMENSIONS / SAMPLES of a scene-txt file (0 for glTF) and the number of ignored NEW_LIGHT blocks."""
        w, h, s, l = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().rt_loaded_info(self._h, C.byref(w), C.byref(h), C.byref(s), C.byref(l)))
        return {"width": w.value, "height": h.value, "samples": s.value, "ignored_lights": l.value}

    def cameras(self) -> list:
        """Every camera of the file as scenegen.Camera (rt_loaded_cameras): glTF camera nodes in the loader's visit order (the last is
        the scene's camera, the one the reference keeps), or the one camera of a scene-txt file."""
        n = C.c_uint32()
        _check(lib().rt_loaded_cameras(self._h, None, 0, C.byref(n)))
        arr = (RtCamera * max(1, n.value))()
        _check(lib().rt_loaded_cameras(self._h, arr, n.value, C.byref(n)))
        return [_camera_from_c(arr[i]) for i in range(n.value)]

    def set_env_map(self, image_path: str, intensity: float = 1.0) -> None:
        """main.cpp:28-31 under USE_ENV_MAP: scene.bg = Texture::load_img(image_path), bg_color = intensity (rt_loaded_set_env_map)."""
        _check(lib().rt_loaded_set_env_map(self._h, os.fsencode(image_path), C.c_float(intensity)))

    def disable_textures(self) -> None:
        """USE_TEXTURES = false (config.h:31-32): every texture lookup returns the texture's first texel (rt_loaded_disable_textures)."""
        _check(lib().rt_loaded_disable_textures(self._h))

    LIGHT_TRIANGLE_RELATIVE_POS = ((10.0, 0.0, -0.1), (0.0, 10.0, -0.1), (0.0, -10.0, -0.1))  # config.h:43-47

    def add_light_triangle(self, rel=LIGHT_TRIANGLE_RELATIVE_POS, intensity: float = 10.0) -> None:
        """scene.h:479-498 under ADD_LIGHT_TRIANGLE: an emissive triangle in the camera's frame (rt_loaded_add_light_triangle)."""
        r = np.ascontiguousarray(rel, dtype=np.float32).reshape(9)
        _check(lib().rt_loaded_add_light_triangle(self._h, fptr(r), C.c_float(intensity)))

    def close(self) -> None:
        if self._h:
            lib().rt_loaded_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _camera_from_c(c: RtCamera) -> "scenegen.Camera":
    return scenegen.Camera(
        position=np.array(list(c.position), dtype=np.float32),
        right=np.array(list(c.right), dtype=np.float32),
        up=np.array(list(c.up), dtype=np.float32),
        forward=np.array(list(c.forward), dtype=np.float32),
        fov_x=float(np.float32(c.fov_x)),
    )


def make_views(cameras, seeds):
    """rt_view[] of scenegen.Camera objects (or anything with position / right / up / forward / fov_x) and one seed per camera."""
    cameras = list(cameras)
    if np.ndim(seeds) == 0:
        seeds = [int(seeds)] * len(cameras)
    seeds = list(seeds)
    if len(seeds) != len(cameras):
        raise ValueError(f"{len(cameras)} cameras but {len(seeds)} seeds")
    views = (RtView * max(1, len(cameras)))()
    for v, (cam, seed) in enumerate(zip(cameras, seeds)):
        for k in range(3):
            views[v].camera.position[k] = np.float32(cam.position[k])
            views[v].camera.right[k] = np.float32(cam.right[k])
            views[v].camera.up[k] = np.float32(cam.up[k])
            views[v].camera.forward[k] = np.float32(cam.forward[k])
        views[v].camera.fov_x = np.float32(cam.fov_x)
        views[v].seed = int(seed)
    return views


RT_SENSOR_PINHOLE, RT_SENSOR_EQUIRECT, RT_SENSOR_FISHEYE, RT_SENSOR_ORTHOGRAPHIC, RT_SENSOR_THIN_LENS = range(5)


@dataclasses.dataclass
class Sensor:
    """One sensor of DeviceScene.render_sensors / sensor_rays / accumulator(sensor=...) (include/rt_abi.h rt_sensor states the rule of every
    kind): `camera` a scenegen.Camera (or anything with position / right / up / forward / fov_x), `kind` an RT_SENSOR_* value, `seed` the
    RT_RNG_DEVICE seed of the view. Use the constructors."""

    camera: object
    kind: int = RT_SENSOR_PINHOLE
    half_width: float = 0.0
    lens_radius: float = 0.0
    focus_distance: float = 0.0
    seed: int = 0

    @classmethod
    def pinhole(cls, camera, seed: int = 0) -> "Sensor":
        return cls(camera, RT_SENSOR_PINHOLE, seed=seed)

    @classmethod
    def equirect(cls, camera, seed: int = 0) -> "Sensor":
        """The full sphere: the image centre looks along forward, columns grow towards right, the top row looks along up."""
        return cls(camera, RT_SENSOR_EQUIRECT, seed=seed)

    @classmethod
    def fisheye(cls, camera, seed: int = 0) -> "Sensor":
        """Equidistant fisheye, camera.fov_x across the image width."""
        return cls(camera, RT_SENSOR_FISHEYE, seed=seed)

    @classmethod
    def orthographic(cls, camera, half_width: float, seed: int = 0) -> "Sensor":
        return cls(camera, RT_SENSOR_ORTHOGRAPHIC, half_width=half_width, seed=seed)

    @classmethod
    def thin_lens(cls, camera, lens_radius: float, focus_distance: float, seed: int = 0) -> "Sensor":
        return cls(camera, RT_SENSOR_THIN_LENS, lens_radius=lens_radius, focus_distance=focus_distance, seed=seed)


def make_sensors(sensors):
    """rt_sensor[] of Sensor objects (ctypes RtSensor records pass through)."""
    sensors = list(sensors)
    out = (RtSensor * max(1, len(sensors)))()
    for v, sn in enumerate(sensors):
        if isinstance(sn, RtSensor):
            C.memmove(C.byref(out[v]), C.byref(sn), C.sizeof(RtSensor))
            continue
        out[v].camera = make_views([sn.camera], 0)[0].camera
        out[v].kind = int(sn.kind)
        out[v].half_width = np.float32(sn.half_width)
        out[v].lens_radius = np.float32(sn.lens_radius)
        out[v].focus_distance = np.float32(sn.focus_distance)
        out[v].seed = int(sn.seed)
    return out


def pack_rays(rays, stream=None, first_sample=None, samples: int = 1, rays_per_output: int = 1) -> np.ndarray:
    """rt_ray records (RAY_DTYPE, contiguous) of what DeviceScene.render_rays accepts: a packed array passes through (a ctypes RtRay array is
    viewed, not copied); an (n, 6) float array gets `stream` / `first_sample`, by default stream = index // rays_per_output and first_sample =
    (index % rays_per_output) x samples."""
    if isinstance(rays, C.Array) and getattr(rays, "_type_", None) is RtRay:
        rays = np.frombuffer(rays, dtype=RAY_DTYPE)
    if isinstance(rays, np.ndarray) and rays.dtype == RAY_DTYPE:
        if stream is not None or first_sample is not None:
            raise ValueError("packed rays carry their own stream / first_sample")
        return np.ascontiguousarray(rays).reshape(-1)
    od = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = od.shape[0]
    idx = np.arange(n, dtype=np.uint64)
    g = max(1, int(rays_per_output))
    out = np.zeros(n, dtype=RAY_DTYPE)
    out["origin"], out["dir"] = od[:, :3], od[:, 3:]
    out["stream"] = (idx // g).astype(np.uint32) if stream is None else np.asarray(stream, dtype=np.uint32).reshape(n)
    out["first_sample"] = ((idx % g) * np.uint64(samples)).astype(np.uint32) if first_sample is None else np.asarray(first_sample, dtype=np.uint32).reshape(n)
    return out


def pack_bake_points(positions, normals=None, stream=None) -> np.ndarray:
    """rt_bake_point records (BAKE_POINT_DTYPE, contiguous) of what DeviceScene.bake_irradiance / bake_sh / bake_rays accept: a packed array
    passes through (a ctypes RtBakePoint array is viewed, not copied); (n, 3) `positions` get `normals` (default: zeros, which bake_sh does
    not read) and `stream` (default: the index)."""
    if isinstance(positions, C.Array) and getattr(positions, "_type_", None) is RtBakePoint:
        positions = np.frombuffer(positions, dtype=BAKE_POINT_DTYPE)
    if isinstance(positions, np.ndarray) and positions.dtype == BAKE_POINT_DTYPE:
        if normals is not None or stream is not None:
            raise ValueError("packed bake points carry their own normal / stream")
        return np.ascontiguousarray(positions).reshape(-1)
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    n = pos.shape[0]
    out = np.zeros(n, dtype=BAKE_POINT_DTYPE)
    out["position"] = pos
    if normals is not None:
        out["normal"] = np.asarray(normals, dtype=np.float32).reshape(n, 3)
    out["stream"] = np.arange(n, dtype=np.uint32) if stream is None else np.asarray(stream, dtype=np.uint32).reshape(n)
    return out


def parse_gltf_scene(path: str, aspect: float) -> LoadedScene:
    h = C.c_void_p()
    _check(lib().rt_gltf_load(os.fsencode(path), C.c_float(aspect), C.byref(h)))
    return LoadedScene(h)


def parse_scene_txt(path: str) -> LoadedScene:
    """The scene-txt front end (csrc/host/txt_loader.cpp): sample_data-style scene files -> triangles + analytic primitives."""
    h = C.c_void_p()
    _check(lib().rt_txt_load(os.fsencode(path), C.byref(h)))
    return LoadedScene(h)


def load_scene(path: str, aspect: float) -> LoadedScene:
    """What the CLI does: scene-txt for *.txt, glTF otherwise (rt_scene_load)."""
    h = C.c_void_p()
    _check(lib().rt_scene_load(os.fsencode(path), C.c_float(aspect), C.byref(h)))
    return LoadedScene(h)


def _as_desc(scene) -> Tuple[RtSceneDesc, object]:
    if isinstance(scene, LoadedScene):
        return scene.desc, scene
    if isinstance(scene, RtSceneDesc):
        return scene, None
    if isinstance(scene, dict):  # an arrays dict (LoadedScene.arrays(), or just the five per-triangle arrays for update_geometry)
        if "camera" in scene:
            scene = scenegen.scene_from_arrays(scene)
        else:
            zero = np.zeros(3, dtype=np.float32)
            n = np.asarray(scene["positions"]).size // 9
            nrm = scene.get("normals")
            scene = scenegen.Scene(positions=np.asarray(scene["positions"], dtype=np.float32).reshape(n, 3, 3), normals=None if nrm is None else np.asarray(nrm),
                                   texcoords=scene["texcoords"], tangents=scene["tangents"], material_ids=scene["material_ids"], materials=[],
                                   camera=scenegen.Camera(zero, zero, zero, zero, 1.0))
    holder = DescHolder(scene)
    return holder.desc, holder


GEOMETRY_ARRAYS = (("positions", 9, np.float32), ("normals", 9, np.float32), ("texcoords", 6, np.float32), ("tangents", 9, np.float32), ("material_ids", 1, np.uint32))


def geometry_arrays(scene) -> dict:
    """The five per-triangle arrays exactly as the library receives them for `scene` (a scenegen.Scene, a LoadedScene or an arrays dict), as
    flat numpy copies keyed positions / normals / texcoords / tangents / material_ids: what _as_desc's descriptor points at, geometric normals
    for normals=None included. DeviceScene.update_geometry(scene) and update_geometry_device(**{on the GPU}) of these are the same update.
    The arrays are read back from the descriptor the one existing path builds (scenegen.DescHolder), so nothing here can drift from it. That
    path normalises given normals in float32, as the reference's loader does: feeding the result through an arrays dict again normalises
    them once more, so geometry_arrays is not a fixed point for normals (the other four arrays are)."""
    desc, keep = _as_desc(scene)  # noqa: F841 (keeps the arrays alive while they are copied)
    n = int(desc.n_triangles)
    out = {}
    for name, per, dtype in GEOMETRY_ARRAYS:
        nbytes = n * per * 4
        out[name] = np.frombuffer(C.string_at(getattr(desc, name), nbytes) if nbytes else b"", dtype=dtype).copy()
    return out


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


class DeviceScene:
    """Device-resident scene + both BVHs: the RaytracerStaticContext of raytracer.h:434-455, in HBM."""

    def __init__(self, scene, device=0, device_bvh: bool = False, wide: bool = False, build_flags: int = 0, **build_options):
        """`device_bvh`: build the scene BVH on the GPU (RT_BUILD_DEVICE_LBVH: production mode, different topology) instead
        of the reference-topology host build. `wide`: collapse that binary tree into the 8-wide quantised tree (RT_BUILD_WIDE:
        production traversal). `build_flags`: further RT_BUILD_* bits; `build_options`: rt_build_options fields by name (device_builder,
        ploc_radius, lbvh_leaf_tris, wide_cost_node, wide_cost_tri). `device`: a HIP ordinal; RT_ALL_DEVICES (-1)
        for one replica per visible GPU + an RCCL communicator; or a list of ordinals (rt_create_on). Multi-GPU scenes shard every render
        over their GPUs and gather on the first one."""
        desc, keep = _as_desc(scene)
        self._keep = keep
        self._accums = []  # live Accumulators: closed before the scene (rt_accum_destroy precedes rt_destroy)
        self._device = None if isinstance(device, (list, tuple)) or int(device) < 0 else int(device)  # the one GPU of a single-GPU scene
        self._h = C.c_void_p()
        if device_bvh or wide or build_flags or build_options:  # a private copy of the descriptor with the build flags set
            d2 = RtSceneDesc()
            C.memmove(C.byref(d2), C.byref(desc), C.sizeof(RtSceneDesc))
            d2.build_flags = int(desc.build_flags) | (RT_BUILD_DEVICE_LBVH if device_bvh else 0) | (RT_BUILD_WIDE if wide else 0) | int(build_flags)
            for k, v in build_options.items():
                if not hasattr(d2.build, k):
                    raise TypeError(f"rt_build_options has no field {k!r}")
                setattr(d2.build, k, v)
            desc = d2
        if isinstance(device, (list, tuple)):
            devs = (C.c_int * len(device))(*[int(d) for d in device])
            _check(lib().rt_create_on(C.byref(desc), devs, len(device), C.byref(self._h)))
        else:
            _check(lib().rt_create(C.byref(desc), int(device), C.byref(self._h)))

    @property
    def n_devices(self) -> int:
        return int(lib().rt_scene_device_count(self._h))

    def close(self) -> None:
        for acc in list(getattr(self, "_accums", [])):
            acc.close()
        if self._h:
            lib().rt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update_geometry(self, scene, refit: bool = False) -> None:
        """rt_update_geometry: new positions, normals, texcoords, tangents and material ids for this scene (same triangle count), from a
        scenegen.Scene, a LoadedScene or an arrays dict, through the path the constructor takes (normals=None: geometric normals).
        Materials, textures, camera and build options stay the scene's. `refit` (RT_BUILD_WIDE scenes): keep the tree's topology and refit
        it on the device (RT_UPDATE_REFIT) instead of rebuilding it."""
        desc, keep = _as_desc(scene)  # noqa: F841 (keeps the arrays alive for the call)
        u = RtGeometryUpdate()
        u.n_triangles = desc.n_triangles
        u.mode = RT_UPDATE_REFIT if refit else RT_UPDATE_REBUILD
        u.positions, u.normals, u.texcoords, u.tangents, u.material_ids = desc.positions, desc.normals, desc.texcoords, desc.tangents, desc.material_ids
        _check(lib().rt_update_geometry(self._h, C.byref(u)))

    def update_geometry_device(self, positions, normals, texcoords, tangents, material_ids, refit: bool = False, n_triangles: Optional[int] = None) -> None:
        """rt_update_geometry_device: update_geometry for arrays that are on this scene's GPU already. Each argument is a contiguous torch
        CUDA tensor (float32; the ids int32 or uint32) of 9 / 9 / 6 / 9 / 1 elements per triangle, or an int device pointer, used with
        `n_triangles`. Normals are required (the geometric-normal default of update_geometry is host code). The tensors are read, not kept
        and not written; torch's current stream on their device is synchronised first, so that they are idle when the library reads them
        on the scene's own stream."""
        import torch

        given = dict(positions=positions, normals=normals, texcoords=texcoords, tangents=tangents, material_ids=material_ids)
        n, device, ptrs = n_triangles, None, {}
        for name, per, dtype in GEOMETRY_ARRAYS:
            a = given[name]
            if isinstance(a, int) and not isinstance(a, bool):
                ptrs[name] = a
                continue
            if not isinstance(a, torch.Tensor) or not a.is_cuda:
                raise TypeError(f"{name}: a torch CUDA tensor or an int device pointer, not {type(a).__name__}" + (" on the CPU" if isinstance(a, torch.Tensor) else ""))
            ok = (torch.float32,) if dtype == np.float32 else tuple(t for t in (torch.int32, getattr(torch, "uint32", None)) if t is not None)
            if a.dtype not in ok:
                raise TypeError(f"{name}: dtype {a.dtype}, expected {' or '.join(str(t) for t in ok)}")
            if not a.is_contiguous():
                raise ValueError(f"{name}: the tensor is not contiguous")
            if a.numel() % per:
                raise ValueError(f"{name}: {a.numel()} elements are no multiple of {per} per triangle")
            if n is None:
                n = a.numel() // per
            if a.numel() != n * per:
                raise ValueError(f"{name}: {a.numel()} elements, expected {n * per} for {n} triangles")
            if device is None:
                device = a.device
            if a.device != device:
                raise ValueError(f"{name}: on {a.device}, the other arrays are on {device}")
            if self._device is not None and a.device.index != self._device:
                raise ValueError(f"{name}: on {a.device}, the scene is on GPU {self._device}")
            ptrs[name] = a.data_ptr() if a.numel() else 0
        if n is None:
            raise ValueError("n_triangles is needed when every array is a device pointer")
        if device is not None:
            torch.cuda.current_stream(device).synchronize()  # the idle precondition
        u = RtGeometryUpdate()
        u.n_triangles = int(n)
        u.mode = RT_UPDATE_REFIT if refit else RT_UPDATE_REBUILD
        for name, _, dtype in GEOMETRY_ARRAYS:
            setattr(u, name, C.cast(C.c_void_p(ptrs[name]), C.POINTER(C.c_float if dtype == np.float32 else C.c_uint32)))
        _check(lib().rt_update_geometry_device(self._h, C.byref(u)))

    def accumulator(self, width: int, height: int, camera=None, seed: int = 0, features: bool = False, sensor=None, ids=None,
                    id_slots: int = 4, light_groups=None, shutter=None, flow=None) -> "Accumulator":
        """A resumable sample accumulator of this scene (rt_accum_create): `camera` a scenegen.Camera (None: the scene's own), `seed` the
        RT_RNG_DEVICE seed. Pixel p of its image is bit for bit run_raytracer(samples = n_p) of that view. `features`: keep the first-hit
        albedo / normal / depth sums as well (rt_accum_create_ex with RT_ACCUM_FEATURES), which features(), read_features() and denoise() need.
        `sensor`: a Sensor in place of `camera` and `seed` (rt_accum_create_sensor): pixel p is then render_sensors(samples = n_p) of it.
        `ids` (not None): Accumulator.attach_ids(ids, slots=id_slots) on the new accumulator, for read_ids(), labels() and matte().
        `light_groups` (not None): Accumulator.attach_light_groups on the new accumulator, for read_light_groups(), light_group() and
        light_mix(): the group of every material (an array), or a dict of attach_light_groups' arguments.
        `shutter` (not None): a dict of Accumulator.attach_shutter's arguments (key0, key1, sensor1, open, close, slices, block, refit): motion
        blur between two geometry keys and two views.
        `flow` (not None): a dict of Accumulator.attach_flow's arguments (key0, key1, sensor1): motion vectors between two geometry keys and
        two views, for flow() and read_flow()."""
        if sensor is not None and camera is not None:
            raise ValueError("accumulator: give a camera or a sensor, not both (the sensor carries its camera and seed)")
        acc = Accumulator(self, width, height, camera, seed, RT_ACCUM_FEATURES if features else 0, sensor=sensor)
        try:
            if ids is not None:
                acc.attach_ids(ids, slots=id_slots)
            if light_groups is not None:
                acc.attach_light_groups(**(light_groups if isinstance(light_groups, dict) else {"material_group": light_groups}))
            if shutter is not None:
                acc.attach_shutter(**shutter)
            if flow is not None:
                acc.attach_flow(**flow)
        except Exception:
            acc.close()
            raise
        return acc

    def render_sensors(self, width: int, height: int, samples: int, sensors, rgb8: bool = False, counters: bool = False, global_best: bool = False,
                       device_out: Optional[int] = None, **tuning):
        """Images of this scene through Sensor objects, one view each, in one call (rt_render_sensors, or rt_render_sensors_rgb8 with `rgb8`):
        pinhole, equirectangular, fisheye, orthographic and thin-lens cameras, evaluated on the device. Returns ((K, H, W, 3) float32 linear
        framebuffers or uint8 images, stats dict); with `device_out` (a device pointer, RT_FLAG_DEVICE_FB) the images stay in HBM and None is
        returned for them. `tuning`: as run_raytracer."""
        sensors = list(sensors)
        recs = make_sensors(sensors)
        k = len(sensors)
        p = RtParams(width, height, samples, RT_RNG_DEVICE, 0, 0, 1, 0, (RT_FLAG_COUNTERS if counters else 0) | (RT_FLAG_GLOBAL_BEST if global_best else 0))
        keep_cb = _apply_tuning(p, tuning)  # noqa: F841
        st = RtStats()
        fn = lib().rt_render_sensors_rgb8 if rgb8 else lib().rt_render_sensors
        if device_out:
            p.flags |= RT_FLAG_DEVICE_FB
            _check(fn(self._h, C.byref(p), recs, k, C.c_void_p(device_out), C.byref(st)))
            return None, st.as_dict()
        img = np.zeros((k, height, width, 3), dtype=np.uint8 if rgb8 else np.float32)
        _check(fn(self._h, C.byref(p), recs, k, img.ctypes.data_as(C.c_void_p), C.byref(st)))
        return img, st.as_dict()

    def sensor_rays(self, sensor, width: int, height: int, samples: int, first_pixel: int = 0, n_pixels: Optional[int] = None, first_sample: int = 0,
                    device_out: Optional[int] = None):
        """The primary rays of a Sensor as the device makes them (rt_sensor_rays): RAY_DTYPE records for samples [first_sample, first_sample +
        samples) of pixels [first_pixel, first_pixel + n_pixels) (default: to the image's end), pixel-major, stream = pixel, first_sample =
        sample index: what render_rays(samples=1, rays_per_output=samples, seed=sensor.seed) turns into render_sensors' image. With
        `device_out` (a device pointer to 32 bytes per record, 16-byte aligned, idle) the records stay in HBM and None is returned."""
        if n_pixels is None:
            n_pixels = int(width) * int(height) - int(first_pixel)
        recs = make_sensors([sensor])
        args = (self._h, recs, int(width), int(height), int(first_pixel), int(n_pixels), int(first_sample), int(samples))
        if device_out:
            _check(lib().rt_sensor_rays(*args, RT_FLAG_DEVICE_FB, C.c_void_p(device_out)))
            return None
        out = np.zeros(int(n_pixels) * int(samples), dtype=RAY_DTYPE)
        _check(lib().rt_sensor_rays(*args, 0, out.ctypes.data_as(C.c_void_p)))
        return out

    def run_raytracer(
        self,
        width: int,
        height: int,
        samples: int,
        rng_mode: int = RT_RNG_DEVICE,
        seed: int = 0,
        shard_index: int = 0,
        shard_count: int = 1,
        shard_block: int = 0,
        out: Optional[np.ndarray] = None,
        device_fb: int = 0,
        counters: bool = False,
        megakernel: bool = False,
        global_best: bool = False,
        **tuning,
    ):
        """run_raytracer(scene, image) (raytracer.h:629): returns (linear float framebuffer (H,W,3), stats dict).
        With `device_fb` (a device pointer) the framebuffer stays in HBM and None is returned for it.
        `counters=True` runs the instrumented kernel variant and fills the event counters of the stats.
        `tuning`: rt_params fields by name — sort_mode (RT_SORT_*), packet_mode (RT_PACKET_*), packet_min_lanes, max_paths,
        progress (a callable (done, total))."""
        p = RtParams(width, height, samples, rng_mode, seed, shard_index, shard_count, shard_block,
                     (RT_FLAG_COUNTERS if counters else 0) | (RT_FLAG_MEGAKERNEL if megakernel else 0) | (RT_FLAG_GLOBAL_BEST if global_best else 0))
        keep_cb = _apply_tuning(p, tuning)  # noqa: F841 (keeps the ctypes callback alive for the call)
        st = RtStats()
        if device_fb:
            p.flags |= RT_FLAG_DEVICE_FB
            _check(lib().rt_render(self._h, C.byref(p), C.c_void_p(device_fb), C.byref(st)))
            return None, st.as_dict()
        fb = out if out is not None else np.zeros((height, width, 3), dtype=np.float32)
        assert fb.dtype == np.float32 and fb.flags["C_CONTIGUOUS"] and fb.size == width * height * 3
        _check(lib().rt_render(self._h, C.byref(p), fb.ctypes.data_as(C.c_void_p), C.byref(st)))
        return fb, st.as_dict()

    def run_raytracer_rgb8(
        self,
        width: int,
        height: int,
        samples: int,
        seed: int = 0,
        shard_index: int = 0,
        shard_count: int = 1,
        shard_block: int = 0,
        out: Optional[np.ndarray] = None,
        device_rgb8: int = 0,
        rng_mode: int = RT_RNG_DEVICE,
        global_best: bool = False,
        **tuning,
    ):
        """run_raytracer(scene, image) with the reference's own output type (image.h:40-42): the tone-mapped rgb8 image,
        film applied on the device. Returns ((H,W,3) uint8 array or None with `device_rgb8`, stats dict). `tuning`: as run_raytracer."""
        p = RtParams(width, height, samples, rng_mode, seed, shard_index, shard_count, shard_block, RT_FLAG_GLOBAL_BEST if global_best else 0)
        keep_cb = _apply_tuning(p, tuning)  # noqa: F841
        st = RtStats()
        if device_rgb8:
            p.flags |= RT_FLAG_DEVICE_FB
            _check(lib().rt_render_rgb8(self._h, C.byref(p), C.c_void_p(device_rgb8), C.byref(st)))
            return None, st.as_dict()
        img = out if out is not None else np.zeros((height, width, 3), dtype=np.uint8)
        assert img.dtype == np.uint8 and img.flags["C_CONTIGUOUS"] and img.size == width * height * 3
        _check(lib().rt_render_rgb8(self._h, C.byref(p), img.ctypes.data_as(C.c_void_p), C.byref(st)))
        return img, st.as_dict()

    def run_raytracer_views(
        self,
        width: int,
        height: int,
        samples: int,
        cameras,
        seeds,
        rgb8: bool = False,
        rng_mode: int = RT_RNG_DEVICE,
        shard_index: int = 0,
        shard_count: int = 1,
        shard_block: int = 0,
        out: Optional[np.ndarray] = None,
        device_fb: int = 0,
        counters: bool = False,
        megakernel: bool = False,
        global_best: bool = False,
        **tuning,
    ):
        """Several camera views of this scene in one call (rt_render_views, or rt_render_views_rgb8 with `rgb8`): `cameras` are
        scenegen.Camera objects, `seeds` one RT_RNG_DEVICE seed per camera (or one for all). Returns ((K, H, W, 3) float32 linear
        framebuffers or uint8 images, or None with `device_fb`, stats dict). View v is bit for bit run_raytracer(...) of a scene created
        with camera v and seed v. Other arguments as run_raytracer."""
        cameras = list(cameras)
        views = make_views(cameras, seeds)
        k = len(cameras)
        p = RtParams(width, height, samples, rng_mode, 0, shard_index, shard_count, shard_block,
                     (RT_FLAG_COUNTERS if counters else 0) | (RT_FLAG_MEGAKERNEL if megakernel else 0) | (RT_FLAG_GLOBAL_BEST if global_best else 0))
        keep_cb = _apply_tuning(p, tuning)  # noqa: F841
        st = RtStats()
        fn = lib().rt_render_views_rgb8 if rgb8 else lib().rt_render_views
        if device_fb:
            p.flags |= RT_FLAG_DEVICE_FB
            _check(fn(self._h, C.byref(p), views, k, C.c_void_p(device_fb), C.byref(st)))
            return None, st.as_dict()
        dt = np.uint8 if rgb8 else np.float32
        img = out if out is not None else np.zeros((k, height, width, 3), dtype=dt)
        assert img.dtype == dt and img.flags["C_CONTIGUOUS"] and img.size == k * width * height * 3
        _check(fn(self._h, C.byref(p), views, k, img.ctypes.data_as(C.c_void_p), C.byref(st)))
        return img, st.as_dict()

    def render_rays(
        self,
        rays,
        stream=None,
        first_sample=None,
        samples: int = 1,
        rays_per_output: int = 1,
        seed: int = 0,
        rgb8: bool = False,
        global_best: bool = False,
        counters: bool = False,
        device_rays: int = 0,
        device_out: int = 0,
        n_rays: Optional[int] = None,
        **tuning,
    ):
        """Radiance along caller-supplied rays (rt_render_rays, or rt_render_rays_rgb8 with `rgb8`). `rays`: an (n, 6) float array
        (origin, dir; directions are used as given) with optional `stream` / `first_sample` arrays (defaults: stream = output index,
        first_sample = (index within the output) x samples, so every sample of an output draws from its own stream position), or a packed
        array: RAY_DTYPE records (what the generators of rays.py return) or a ctypes RtRay array. Ray r draws `samples` samples seeded from
        (seed, stream_r, first_sample_r + s); output j averages rays j * rays_per_output .. in order (include/rt_abi.h states the rule).
        Returns ((n / rays_per_output, 3) float32 or uint8 outputs, stats dict).
        The device form (RT_FLAG_DEVICE_FB): `device_rays` (a device pointer to packed records, 16-byte aligned), `n_rays` (how many records
        it holds: required here, not read otherwise) and `device_out` (a device pointer to n_rays / rays_per_output x 3 floats, or bytes with
        `rgb8`) go together and `rays` is not read; nothing is copied and None is returned for the outputs. Both buffers must be idle.
        `tuning`: as run_raytracer."""
        p = RtParams(0, 0, int(samples), RT_RNG_DEVICE, int(seed), 0, 1, 0, (RT_FLAG_COUNTERS if counters else 0) | (RT_FLAG_GLOBAL_BEST if global_best else 0))
        keep_cb = _apply_tuning(p, tuning)  # noqa: F841
        st = RtStats()
        fn = lib().rt_render_rays_rgb8 if rgb8 else lib().rt_render_rays
        g = int(rays_per_output)
        if bool(device_rays) != bool(device_out):
            raise ValueError("render_rays: device_rays and device_out go together (RT_FLAG_DEVICE_FB covers both buffers)")
        if device_rays:
            if n_rays is None:
                raise ValueError("render_rays: device_rays needs n_rays")
            p.flags |= RT_FLAG_DEVICE_FB
            _check(fn(self._h, C.byref(p), C.c_void_p(device_rays), int(n_rays), g, C.c_void_p(device_out), C.byref(st)))
            return None, st.as_dict()
        packed = pack_rays(rays, stream, first_sample, samples=int(samples), rays_per_output=max(1, g))
        n = len(packed)
        out = np.zeros((n // max(1, g), 3), dtype=np.uint8 if rgb8 else np.float32)
        _check(fn(self._h, C.byref(p), packed.ctypes.data_as(C.c_void_p), n, g, out.ctypes.data_as(C.c_void_p), C.byref(st)))
        return out, st.as_dict()

    def _bake(self, kind, points, samples, seed, offset, first_sample, device_points, n_points, device_out, global_best, counters, tuning):
        p = RtParams(0, 0, int(samples), RT_RNG_DEVICE, int(seed), 0, 1, 0, (RT_FLAG_COUNTERS if counters else 0) | (RT_FLAG_GLOBAL_BEST if global_best else 0))
        keep_cb = _apply_tuning(p, tuning)  # noqa: F841
        b = RtBake(int(kind), int(first_sample) & 0xFFFFFFFF, float(offset))
        st = RtStats()
        shape = (9, 3) if kind == RT_BAKE_SH9 else (3,)
        if bool(device_points) != bool(device_out):
            raise ValueError("bake: device_points and device_out go together (RT_FLAG_DEVICE_FB covers both buffers)")
        if device_points:
            if n_points is None:
                raise ValueError("bake: device_points needs n_points")
            p.flags |= RT_FLAG_DEVICE_FB
            _check(lib().rt_bake(self._h, C.byref(p), C.byref(b), C.c_void_p(device_points), int(n_points), C.c_void_p(device_out), C.byref(st)))
            return None, st.as_dict()
        packed = pack_bake_points(points)
        out = np.zeros((len(packed),) + shape, dtype=np.float32)
        _check(lib().rt_bake(self._h, C.byref(p), C.byref(b), packed.ctypes.data_as(C.c_void_p), len(packed), out.ctypes.data_as(C.c_void_p), C.byref(st)))
        return out, st.as_dict()

    def bake_irradiance(self, points, samples: int, seed: int = 0, offset: float = 0.0, first_sample: int = 0, device_points: Optional[int] = None,
                        n_points: Optional[int] = None, device_out: Optional[int] = None, global_best: bool = False, counters: bool = False, **tuning):
        """Irradiance at surface points (rt_bake, RT_BAKE_IRRADIANCE): `points` are BAKE_POINT_DTYPE records (pack_bake_points makes them from
        positions and normals; lightmap_points from an atlas). Sample s of point j is seeded from (seed, stream_j, first_sample + s), leaves
        position + offset * normal along the reference's cosine lobe around the normal and is path-traced as a camera ray is;
        E_j = pi x the mean radiance (include/rt_abi.h states the rule). Returns ((n, 3) float32, stats dict).
        The device form (RT_FLAG_DEVICE_FB): `device_points` (a device pointer to packed records, 16-byte aligned), `n_points` and
        `device_out` (a device pointer to n x 3 floats) go together and `points` is not read; nothing is copied and None is returned for the
        outputs. Both buffers must be idle. `tuning`: as run_raytracer."""
        return self._bake(RT_BAKE_IRRADIANCE, points, samples, seed, offset, first_sample, device_points, n_points, device_out, global_best, counters, tuning)

    def bake_sh(self, points, samples: int, seed: int = 0, first_sample: int = 0, device_points: Optional[int] = None, n_points: Optional[int] = None,
                device_out: Optional[int] = None, global_best: bool = False, counters: bool = False, **tuning):
        """Spherical-harmonic light probes (rt_bake, RT_BAKE_SH9): the radiance arriving at each point from the whole sphere, projected on the
        nine real SH basis functions of bands 0..2 in the order rt_abi.h lists them. Normals are not read. Returns ((n, 9, 3) float32, stats
        dict); the device form is bake_irradiance's with n x 27 floats of output."""
        return self._bake(RT_BAKE_SH9, points, samples, seed, 0.0, first_sample, device_points, n_points, device_out, global_best, counters, tuning)

    def bake_rays(self, points, samples: int, seed: int = 0, sh: bool = False, offset: float = 0.0, first_sample: int = 0, device_points: Optional[int] = None,
                  n_points: Optional[int] = None, device_out: Optional[int] = None):
        """The first rays of a bake as the device makes them (rt_bake_rays): RAY_DTYPE records for samples [first_sample, first_sample +
        samples) of every point, point-major, stream = the point's, first_sample = the sample index: what render_rays(samples=1,
        rays_per_output=samples, seed=seed) turns into bake_irradiance / pi. `sh`: the rays of bake_sh. With `device_points`, `n_points` and
        `device_out` (device pointers, 16-byte aligned, idle; 32 bytes per record) the records stay in HBM and None is returned."""
        b = RtBake(RT_BAKE_SH9 if sh else RT_BAKE_IRRADIANCE, int(first_sample) & 0xFFFFFFFF, float(offset))
        if bool(device_points) != bool(device_out):
            raise ValueError("bake_rays: device_points and device_out go together (RT_FLAG_DEVICE_FB covers both buffers)")
        if device_points:
            if n_points is None:
                raise ValueError("bake_rays: device_points needs n_points")
            _check(lib().rt_bake_rays(self._h, C.byref(b), int(seed), C.c_void_p(device_points), int(n_points), int(samples), RT_FLAG_DEVICE_FB, C.c_void_p(device_out)))
            return None
        packed = pack_bake_points(points)
        out = np.zeros(len(packed) * int(samples), dtype=RAY_DTYPE)
        _check(lib().rt_bake_rays(self._h, C.byref(b), int(seed), packed.ctypes.data_as(C.c_void_p), len(packed), int(samples), 0, out.ctypes.data_as(C.c_void_p)))
        return out

    def lightmap_points(self, positions, normals, lm_uv, width: int, height: int, capacity: Optional[int] = None, n_triangles: Optional[int] = None,
                        device_points: Optional[int] = None, device_texels: Optional[int] = None):
        """The covered texel centres of a width x height light-map atlas as bake points (rt_lightmap_points): `positions` / `normals` (9 floats
        per triangle) and `lm_uv` (6: the corners' atlas coordinates in [0, 1]^2). A texel belongs to the lowest triangle whose atlas
        triangle holds its centre (edges included); its point is the interpolated position and normalised normal, stream = texel index.
        Returns (points (BAKE_POINT_DTYPE), texels (uint32: y * width + x)) in increasing texel order; scatter a bake's rows to
        image.reshape(-1, 3)[texels]. With `capacity` at most that many are written (the first ones) and the number of owned texels is
        returned as a third element.
        The device form (RT_FLAG_DEVICE_FB): the three arrays are contiguous float32 torch CUDA tensors (or int device pointers, with
        `n_triangles`), `device_points` / `device_texels` device pointers with room for `capacity` records (points 16-byte aligned); all idle.
        Returns the count of owned texels."""
        cap = int(width) * int(height) if capacity is None else int(capacity)
        count = C.c_uint32()
        if device_points or device_texels:
            ptrs, n = [], n_triangles
            for name, a, per in (("positions", positions, 9), ("normals", normals, 9), ("lm_uv", lm_uv, 6)):
                if isinstance(a, int) and not isinstance(a, bool):
                    ptrs.append(a)
                    continue
                import torch

                if not isinstance(a, torch.Tensor) or not a.is_cuda or a.dtype != torch.float32 or not a.is_contiguous():
                    raise TypeError(f"{name}: a contiguous float32 torch CUDA tensor or an int device pointer")
                if n is None:
                    n = a.numel() // per
                if a.numel() != n * per:
                    raise ValueError(f"{name}: {a.numel()} elements, expected {n * per} for {n} triangles")
                torch.cuda.current_stream(a.device).synchronize()  # the idle precondition
                ptrs.append(a.data_ptr() if a.numel() else 0)
            if n is None:
                raise ValueError("n_triangles is needed when every array is a device pointer")
            _check(lib().rt_lightmap_points(self._h, *(C.c_void_p(q) for q in ptrs), int(n), int(width), int(height), RT_FLAG_DEVICE_FB,
                                            C.c_void_p(device_points), C.c_void_p(device_texels), cap, C.byref(count)))
            return int(count.value)
        pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 9)
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 9)
        uv = np.ascontiguousarray(lm_uv, dtype=np.float32).reshape(-1, 6)
        if not (len(pos) == len(nrm) == len(uv)):
            raise ValueError(f"lightmap_points: {len(pos)} / {len(nrm)} / {len(uv)} triangles in positions / normals / lm_uv")
        pts = np.zeros(max(cap, 1), dtype=BAKE_POINT_DTYPE)
        tex = np.zeros(max(cap, 1), dtype=np.uint32)
        _check(lib().rt_lightmap_points(self._h, pos.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p), len(pos), int(width),
                                        int(height), 0, pts.ctypes.data_as(C.c_void_p), tex.ctypes.data_as(C.c_void_p), cap, C.byref(count)))
        k = min(int(count.value), cap)
        return (pts[:k].copy(), tex[:k].copy()) if capacity is None else (pts[:k].copy(), tex[:k].copy(), int(count.value))

    def film_rgb8(self, fb: np.ndarray) -> np.ndarray:
        """The device film (image.h:49-82 on the GPU) applied to a host float array of shape (..., 3)."""
        fb = np.ascontiguousarray(fb, dtype=np.float32)
        out = np.zeros(fb.shape, dtype=np.uint8)
        _check(lib().rt_film_rgb8(self._h, fptr(fb), fb.size // 3, u8ptr(out)))
        return out

    def cast_rays(self, rays: np.ndarray):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        prim = np.zeros(n, dtype=np.uint32)
        bct = np.zeros((n, 3), dtype=np.float32)
        _check(lib().rt_cast_rays(self._h, fptr(rays), n, u32ptr(prim), fptr(bct)))
        return prim, bct

    def cast_rays_ex(self, rays: np.ndarray, mode: int):
        """rt_cast_rays_ex: the closest-hit probe through the renderer's own kernels (mode = RT_CAST_*).
        Returns (prim, bct, stats dict with casts / nodes_visited / box_tests / tri_tests / kernel_ms)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        prim = np.zeros(n, dtype=np.uint32)
        bct = np.zeros((n, 3), dtype=np.float32)
        st = RtStats()
        _check(lib().rt_cast_rays_ex(self._h, fptr(rays), n, int(mode), u32ptr(prim), fptr(bct), C.byref(st)))
        return prim, bct, st.as_dict()

    def surface_normals(self, rays: np.ndarray):
        """rt_surface_normals: closest hit + the normals to_intersection_info (bvh.h:80-121) hands to shade().
        Returns (prim, t, normal (n,3), shading_normal (n,3))."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        prim = np.zeros(n, dtype=np.uint32)
        t = np.zeros(n, dtype=np.float32)
        nn = np.zeros((n, 3), dtype=np.float32)
        sn = np.zeros((n, 3), dtype=np.float32)
        _check(lib().rt_surface_normals(self._h, fptr(rays), n, u32ptr(prim), fptr(t), fptr(nn), fptr(sn)))
        return prim, t, nn, sn

    def light_pdf(self, rays: np.ndarray) -> np.ndarray:
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        out = np.zeros(n, dtype=np.float32)
        _check(lib().rt_light_pdf(self._h, fptr(rays), n, fptr(out)))
        return out

    def bg_at(self, dirs: np.ndarray) -> np.ndarray:
        """Scene::bg_at (scene.h:83-89) for explicit directions -> (n, 3) rgb (rt_bg_at)."""
        dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = dirs.shape[0]
        out = np.zeros((n, 3), dtype=np.float32)
        _check(lib().rt_bg_at(self._h, fptr(dirs), n, fptr(out)))
        return out

    def set_environment(self, rgb: Optional[np.ndarray], importance: bool = False) -> None:
        """rt_set_environment: an (H, W, 3) float32 array of linear radiance (row 0 = the +y pole; finite, >= 0) becomes this scene's
        background for every wavefront entry point and for bg_at, in place of the 8-bit bg_texture; `importance` adds RT_ENV_IMPORTANCE:
        shade()'s mix_dist samples the map. None: back to what the scene was created with. The array is copied."""
        if rgb is None:
            _check(lib().rt_set_environment(self._h, None))
            return
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("set_environment: expected an (H, W, 3) array")
        e = RtEnvironment()
        e.height, e.width = rgb.shape[0], rgb.shape[1]
        e.rgb = fptr(rgb)
        e.flags = RT_ENV_IMPORTANCE if importance else 0
        _check(lib().rt_set_environment(self._h, C.byref(e)))

    def env_pdf(self, dirs: np.ndarray) -> np.ndarray:
        """rt_env_pdf: the solid-angle pdf of the environment distribution for (n, 3) directions, from the device's own tables."""
        dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(dirs.shape[0], dtype=np.float32)
        _check(lib().rt_env_pdf(self._h, fptr(dirs), dirs.shape[0], fptr(out)))
        return out

    def env_sample(self, xi: np.ndarray) -> np.ndarray:
        """rt_env_sample: the directions (n, 3) the environment sampler makes of (n, 4) uniforms in [0, 1)."""
        xi = np.ascontiguousarray(xi, dtype=np.float32).reshape(-1, 4)
        out = np.zeros((xi.shape[0], 3), dtype=np.float32)
        _check(lib().rt_env_sample(self._h, fptr(xi), xi.shape[0], fptr(out)))
        return out

    def bvh_device_dump(self, which: int = 0):
        """The BVH as the kernels see it, read back from HBM: {root, nodes (n_inner,16) u32, tris (n_tris,12) u32}."""
        ni, nt, root = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().rt_bvh_device_dump(self._h, which, C.byref(ni), C.byref(nt), C.byref(root), None, None))
        nodes = np.zeros((ni.value, 16), dtype=np.uint32)
        tris = np.zeros((nt.value, 12), dtype=np.uint32)
        _check(lib().rt_bvh_device_dump(self._h, which, C.byref(ni), C.byref(nt), C.byref(root), u32ptr(nodes), u32ptr(tris)))
        return {"root": root.value, "nodes": nodes, "tris": tris}

    def bvh_wide_dump(self):
        """The 8-wide scene BVH read back from HBM: {depth, nodes (n,20) u32 (WideNode records), tris (n_tris,12) u32}."""
        nn, nt, dp = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().rt_bvh_wide_dump(self._h, C.byref(nn), C.byref(nt), C.byref(dp), None, None))
        nodes = np.zeros((nn.value, 20), dtype=np.uint32)
        tris = np.zeros((nt.value, 12), dtype=np.uint32)
        _check(lib().rt_bvh_wide_dump(self._h, C.byref(nn), C.byref(nt), C.byref(dp), u32ptr(nodes), u32ptr(tris)))
        return {"depth": dp.value, "nodes": nodes, "tris": tris}

    def build_times(self):
        b, u, w = C.c_double(), C.c_double(), C.c_double()
        _check(lib().rt_build_times_ex(self._h, C.byref(b), C.byref(u), C.byref(w)))
        return {"build_ms": b.value, "upload_ms": u.value, "wide_ms": w.value}

    def refit_times(self):
        """rt_refit_times: wall ms of the last refit on the device, and of its top-down level pass."""
        r, l = C.c_double(), C.c_double()
        _check(lib().rt_refit_times(self._h, C.byref(r), C.byref(l)))
        return {"refit_ms": r.value, "levels_ms": l.value}

    def bvh_info(self, which: int):
        nn, no, root = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().rt_bvh_info(self._h, which, C.byref(nn), C.byref(no), C.byref(root), None, None))
        nodes = np.zeros((nn.value, 10), dtype=np.uint32)
        order = np.zeros(no.value, dtype=np.uint32)
        _check(lib().rt_bvh_info(self._h, which, C.byref(nn), C.byref(no), C.byref(root), u32ptr(nodes), u32ptr(order)))
        return {"root": root.value, "nodes": nodes, "order": order}


class Accumulator:
    """Progressive and adaptive rendering (include/rt_abi.h rt_accum_*): per-pixel sums S, E (even-index samples) and counts n that
    survive between calls. Keeps its DeviceScene alive; DeviceScene.close() closes it first."""

    def __init__(self, scene: DeviceScene, width: int, height: int, camera=None, seed: int = 0, accum_flags: int = 0, sensor=None):
        self._scene = scene
        self.width, self.height = int(width), int(height)
        self.id_slots = self.n_light_groups = 1  # K of read_ids(), G of the light-group reads: 1 until attach_ids / attach_light_groups
        self._h = C.c_void_p()
        if sensor is not None:
            _check(lib().rt_accum_create_sensor(scene._h, self.width, self.height, make_sensors([sensor]), int(accum_flags), C.byref(self._h)))
            scene._accums.append(self)
            return
        cam = None
        if camera is not None:
            cam = make_views([camera], 0)[0].camera
        cam_p = C.byref(cam) if cam is not None else None
        if accum_flags:
            _check(lib().rt_accum_create_ex(scene._h, self.width, self.height, cam_p, int(seed), int(accum_flags), C.byref(self._h)))
        else:
            _check(lib().rt_accum_create(scene._h, self.width, self.height, cam_p, int(seed), C.byref(self._h)))
        scene._accums.append(self)

    def _params(self, samples: int, global_best: bool, counters: bool, tuning: dict):
        p = RtParams(self.width, self.height, samples, RT_RNG_DEVICE, 0, 0, 1, 0,
                     (RT_FLAG_GLOBAL_BEST if global_best else 0) | (RT_FLAG_COUNTERS if counters else 0))
        return p, _apply_tuning(p, tuning)

    def _zeros(self, dtype, *tail) -> np.ndarray:
        return np.zeros((self.height, self.width) + tail, dtype=dtype)

    def _state(self, call, **arrays) -> dict:
        """name -> a zeroed (H, W, *tail) array per `arrays` (name=(dtype, *tail)), filled by call(*pointers) in that order."""
        out = {k: self._zeros(*spec) for k, spec in arrays.items()}
        _check(call(*[(fptr if a.dtype == np.float32 else u32ptr)(a) for a in out.values()]))
        return out

    def _output(self, call, dtype=np.float32, tail=(3,), device_out=None):
        """The one output of call(flags, pointer): a new (H, W, *tail) array, or with `device_out` (a device pointer, RT_FLAG_DEVICE_FB) None."""
        if device_out:
            _check(call(RT_FLAG_DEVICE_FB, C.c_void_p(device_out)))
            return None
        out = self._zeros(dtype, *tail)
        _check(call(0, out.ctypes.data_as(C.c_void_p)))
        return out

    def render(self, samples: int, global_best: bool = False, counters: bool = False, **tuning) -> dict:
        """rt_accum_render: `samples` more samples for every pixel. `tuning`: as DeviceScene.run_raytracer. Returns the stats dict."""
        p, keep_cb = self._params(samples, global_best, counters, tuning)  # noqa: F841
        st = RtStats()
        _check(lib().rt_accum_render(self._h, C.byref(p), C.byref(st)))
        return st.as_dict()

    def render_adaptive(self, threshold: float, min_samples: int = 16, max_samples: int = 256, step: int = 32, global_best: bool = False,
                        counters: bool = False, **tuning) -> dict:
        """rt_accum_render_adaptive: rounds of `step` samples for the pixels whose 3x3 window holds an error above `threshold`, until none
        does or they reach `max_samples`. Returns the stats dict with "rounds"."""
        p, keep_cb = self._params(0, global_best, counters, tuning)  # noqa: F841
        ad = RtAdaptive(float(threshold), int(min_samples), int(max_samples), int(step))
        st = RtStats()
        rounds = C.c_uint32(0)
        _check(lib().rt_accum_render_adaptive(self._h, C.byref(p), C.byref(ad), C.byref(rounds), C.byref(st)))
        d = st.as_dict()
        d["rounds"] = int(rounds.value)
        return d

    def image(self, rgb8: bool = False) -> np.ndarray:
        """The resolved image S / n: (H, W, 3) float32, or the device film's uint8 image with `rgb8`."""
        fn = lib().rt_accum_resolve_rgb8 if rgb8 else lib().rt_accum_resolve
        return self._output(lambda flags, p: fn(self._h, flags, p), np.uint8 if rgb8 else np.float32)

    def read(self) -> dict:
        """The state: "sum" and "even_sum" (H, W, 3) float32, "samples" (H, W) uint32, "error" (H, W) float32 (the last judge's)."""
        return self._state(lambda *p: lib().rt_accum_read(self._h, *p), sum=(np.float32, 3), even_sum=(np.float32, 3), samples=(np.uint32,), error=(np.float32,))

    def read_features(self) -> dict:
        """The raw first-hit sums (rt_accum_read_features): "albedo_sum" and "normal_sum" (H, W, 3) float32, "depth_sum" (H, W) float32,
        "hits" (H, W) uint32. Needs accumulator(features=True)."""
        return self._state(lambda *p: lib().rt_accum_read_features(self._h, *p), albedo_sum=(np.float32, 3), normal_sum=(np.float32, 3), depth_sum=(np.float32,),
                           hits=(np.uint32,))

    def features(self) -> dict:
        """The feature means (rt_accum_resolve_features): "albedo" = AS / n and "normal" = NS / n (not renormalised), (H, W, 3) float32;
        "depth" = ZS / h (0 where no sample hit), (H, W) float32."""
        return self._state(lambda *p: lib().rt_accum_resolve_features(self._h, 0, *p), albedo=(np.float32, 3), normal=(np.float32, 3), depth=(np.float32,))

    def denoise(self, rgb8: bool = False, **opts) -> np.ndarray:
        """rt_accum_denoise: the image filtered by the edge-avoiding a-trous filter that the feature means and the half-buffer noise estimate
        guide; the accumulator is not modified. `opts`: rt_denoise fields by name (iterations, sigma_color, sigma_depth, normal_sharpness,
        flags, reserved) or demodulate=False for RT_DENOISE_NO_DEMODULATE. (H, W, 3) float32, or the device film's uint8 image with `rgb8`."""
        o = RtDenoise()
        for k, v in opts.items():
            if k == "demodulate":
                if not v:
                    o.flags |= RT_DENOISE_NO_DEMODULATE
            elif k == "reserved":
                for i, r in enumerate(v):
                    o.reserved[i] = int(r)
            elif k in ("sigma_color", "sigma_depth"):
                setattr(o, k, float(v))
            elif k in ("iterations", "normal_sharpness", "flags"):
                setattr(o, k, int(v) | (o.flags if k == "flags" else 0))
            else:
                raise TypeError(f"rt_denoise has no field {k!r}")
        fn = lib().rt_accum_denoise_rgb8 if rgb8 else lib().rt_accum_denoise
        return self._output(lambda flags, p: fn(self._h, C.byref(o), flags, p), np.uint8 if rgb8 else np.float32)

    def attach_ids(self, kind="primitive", slots: int = 4, n_table: Optional[int] = None) -> None:
        """rt_accum_attach_ids: keep, per pixel, a table of `slots` (id, count) pairs of the ids its samples' primary rays hit, first seen first,
        and a count of the samples that found the table full. `kind`: "primitive" (what cast_rays reports), "material", or a table of user
        ids, one per original triangle and then per analytic primitive: a uint32 array (copied), or a device pointer (an int, with `n_table`
        entries; RT_FLAG_DEVICE_FB). Once, before the first render."""
        d = RtIdDesc()
        d.slots = int(slots)
        keep = None
        if isinstance(kind, str):
            if kind not in ("primitive", "material"):
                raise ValueError(f"attach_ids: kind {kind!r} is not 'primitive', 'material', an array or a device pointer")
            d.kind = RT_ID_PRIMITIVE if kind == "primitive" else RT_ID_MATERIAL
        elif isinstance(kind, (int, np.integer)):
            if n_table is None:
                raise ValueError("attach_ids: a device pointer needs n_table")
            d.kind, d.table, d.n_table, d.flags = RT_ID_USER, int(kind), int(n_table), RT_FLAG_DEVICE_FB
        else:
            keep = np.ascontiguousarray(kind, dtype=np.uint32).reshape(-1)
            d.kind, d.table, d.n_table = RT_ID_USER, keep.ctypes.data, keep.size
        _check(lib().rt_accum_attach_ids(self._h, C.byref(d)))
        self.id_slots = int(d.slots) if d.slots else 4

    def read_ids(self) -> dict:
        """The id tables (rt_accum_read_ids): "ids" and "counts" (H, W, K) uint32 in first-seen order (an empty slot reads id 0, count 0),
        "other" (H, W) uint32: the samples no slot was left for. Needs attach_ids."""
        return self._state(lambda *p: lib().rt_accum_read_ids(self._h, *p), ids=(np.uint32, self.id_slots), counts=(np.uint32, self.id_slots), other=(np.uint32,))

    def labels(self, device_out=None):
        """rt_accum_resolve_labels: (label (H, W) uint32: the id of each pixel's fullest slot, RT_ID_MISS where n = 0; coverage (H, W) float32:
        that slot's count / n). `device_out`: a pair of device pointers (label, coverage; either may be None or 0) that receive them in HBM
        (RT_FLAG_DEVICE_FB); then (None, None) is returned."""
        if device_out is not None:
            lp, cp = device_out
            _check(lib().rt_accum_resolve_labels(self._h, RT_FLAG_DEVICE_FB, C.c_void_p(lp or None), C.c_void_p(cp or None)))
            return None, None
        return tuple(self._state(lambda *p: lib().rt_accum_resolve_labels(self._h, 0, *p), label=(np.uint32,), coverage=(np.float32,)).values())

    def matte(self, ids, device_out: Optional[int] = None):
        """rt_accum_resolve_matte: (H, W) float32, the share of each pixel's samples whose id is one of `ids` (1..4096 of them; duplicates count
        once), as far as the pixel's slots hold it. `device_out`: a device pointer that receives it in HBM; then None is returned."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        return self._output(lambda flags, p: lib().rt_accum_resolve_matte(self._h, flags, u32ptr(ids), ids.size, p), tail=(), device_out=device_out)

    def attach_light_groups(self, material_group, background=None, n_groups: Optional[int] = None, n_materials: Optional[int] = None) -> None:
        """rt_accum_attach_light_groups: keep, per pixel, one more sum for each of `n_groups` light groups (1..8): the part of the pixel's
        radiance that the emitters of the group produced. `material_group`: the group of every material of the scene, None or
        RT_LIGHT_GROUP_NONE for a material in no group: a sequence (copied), or a device pointer to uint32 words (an int, with `n_materials`;
        RT_FLAG_DEVICE_FB). `background`: the group of the background or environment, None for none. `n_groups`: by default one more than the
        largest group named. Once, before the first render."""
        d = RtLightGroupDesc()
        none = RT_LIGHT_GROUP_NONE
        d.background_group = none if background is None else int(background)
        keep = None
        named = [] if background is None else [int(background)]
        if isinstance(material_group, (int, np.integer)):
            if n_materials is None or n_groups is None:
                raise ValueError("attach_light_groups: a device pointer needs n_materials and n_groups")
            d.material_group, d.n_materials, d.flags = int(material_group), int(n_materials), RT_FLAG_DEVICE_FB
        else:
            keep = np.array([none if g is None else int(g) for g in material_group], dtype=np.uint32)
            d.material_group, d.n_materials = keep.ctypes.data, keep.size
            named += [int(g) for g in keep if g != none]
        d.n_groups = int(n_groups) if n_groups is not None else max(named, default=0) + 1
        _check(lib().rt_accum_attach_light_groups(self._h, C.byref(d)))
        self.n_light_groups = int(d.n_groups)

    def read_light_groups(self) -> np.ndarray:
        """The group sums GS (rt_accum_read_light_groups): (G, H, W, 3) float32, GS[g] the sum over each pixel's samples of the part of their
        radiance that group g's emitters produced. Needs attach_light_groups."""
        out = np.zeros((self.n_light_groups, self.height, self.width, 3), dtype=np.float32)
        _check(lib().rt_accum_read_light_groups(self._h, fptr(out)))
        return out

    def light_group(self, g: int, device_out: Optional[int] = None):
        """rt_accum_resolve_light_group: the image of group g alone, GS[g] / n: (H, W, 3) float32. `device_out`: a device pointer that
        receives it in HBM (RT_FLAG_DEVICE_FB); then None is returned."""
        return self._output(lambda flags, p: lib().rt_accum_resolve_light_group(self._h, int(g), flags, p), device_out=device_out)

    def light_mix(self, weights, rgb8: bool = False, device_out: Optional[int] = None):
        """rt_accum_resolve_light_mix: the image relit, sum over g of (GS[g] / n) * weights[g]: `weights` is (G, 3), or (G,) for one factor per
        group. (H, W, 3) float32, or the device film's uint8 image with `rgb8`. `device_out`: a device pointer that receives it in HBM
        (RT_FLAG_DEVICE_FB); then None is returned."""
        G = self.n_light_groups
        w = np.asarray(weights, dtype=np.float32)
        if w.shape == (G,):
            w = np.repeat(w[:, None], 3, axis=1)
        if w.shape != (G, 3):
            raise ValueError(f"light_mix: weights must have shape ({G}, 3) or ({G},), not {w.shape}")
        w = np.ascontiguousarray(w)
        fn = lib().rt_accum_resolve_light_mix_rgb8 if rgb8 else lib().rt_accum_resolve_light_mix
        return self._output(lambda flags, p: fn(self._h, fptr(w), flags, p), np.uint8 if rgb8 else np.float32, device_out=device_out)

    def attach_shutter(self, key0=None, key1=None, sensor1=None, open: float = 0.0, close: float = 1.0, slices: int = 16, block: int = 4,
                       refit: bool = True, reserved=None) -> None:
        """rt_accum_attach_shutter (include/rt_abi.h states the rule): sample s is rendered at time t_k of slice k = bitreverse((s // block) %
        slices), on the scene blended between `key0` (t = 0) and `key1` (t = 1) and through the view blended between the accumulator's own and
        `sensor1` (a Sensor of the same kind; None: the view does not move). A key is a scenegen.Scene, a LoadedScene or an arrays dict as
        update_geometry takes them, or a dict of contiguous torch CUDA tensors (positions, normals, texcoords, tangents, material_ids) as
        update_geometry_device takes them; both keys of one kind. Texcoords and material ids are key 0's. Both keys None: a camera-only
        shutter, the geometry is never touched. `refit`: install a slice with RT_UPDATE_REFIT (RT_BUILD_WIDE scenes) instead of
        RT_UPDATE_REBUILD. Once, before the first render; afterwards and after every render the scene is key 0's."""
        d = RtShutterDesc()
        d.mode = RT_UPDATE_REFIT if refit else RT_UPDATE_REBUILD
        d.open, d.close, d.slices, d.block = float(open), float(close), int(slices), int(block)
        for i, r in enumerate(reserved or ()):
            d.reserved[i] = int(r)
        keep = []
        if (key0 is None) != (key1 is None):
            raise ValueError("attach_shutter: give both geometry keys or neither")
        if key0 is not None:
            keys, on_device = [], None
            for key in (key0, key1):
                dev_key = isinstance(key, dict) and any(hasattr(v, "data_ptr") for v in key.values())
                if on_device is not None and dev_key != on_device:
                    raise ValueError("attach_shutter: one key is on the device and the other is not")
                on_device = dev_key
                if dev_key:
                    import torch

                    for name, per, dtype in GEOMETRY_ARRAYS:
                        a = key[name]
                        if not a.is_cuda or not a.is_contiguous() or (dtype == np.float32 and a.dtype != torch.float32) or a.element_size() != 4:
                            raise TypeError(f"attach_shutter: {name} must be a contiguous 4-byte torch CUDA tensor")
                    torch.cuda.current_stream(key["positions"].device).synchronize()  # the idle precondition
                    keys.append({name: (key[name].data_ptr() if key[name].numel() else 0, key[name].numel() // per) for name, per, _ in GEOMETRY_ARRAYS})
                else:
                    arrays = geometry_arrays(key)
                    keep.append(arrays)
                    keys.append({name: (arrays[name].ctypes.data if arrays[name].size else 0, arrays[name].size // per) for name, per, _ in GEOMETRY_ARRAYS})
            counts = {n for k in keys for _, n in k.values()}
            if len(counts) != 1:
                raise ValueError(f"attach_shutter: the arrays of the keys hold different triangle counts {sorted(counts)}")
            d.n_triangles = counts.pop()
            d.flags = RT_FLAG_DEVICE_FB if on_device else 0
            for i in range(2):
                d.positions[i], d.normals[i], d.tangents[i] = keys[i]["positions"][0], keys[i]["normals"][0], keys[i]["tangents"][0]
            d.texcoords, d.material_ids = keys[0]["texcoords"][0], keys[0]["material_ids"][0]
        if sensor1 is not None:
            rec = make_sensors([sensor1])
            keep.append(rec)
            d.sensor1 = C.cast(rec, C.POINTER(RtSensor))
        _check(lib().rt_accum_attach_shutter(self._h, C.byref(d)))

    def shutter_times(self) -> dict:
        """rt_accum_shutter_times: of the last render() call, "slice_changes" (the slices it installed) and "slice_change_ms" (their wall time
        in all)."""
        ms, n = C.c_double(0), C.c_uint32(0)
        _check(lib().rt_accum_shutter_times(self._h, C.byref(ms), C.byref(n)))
        return {"slice_change_ms": float(ms.value), "slice_changes": int(n.value)}

    def shutter_info(self) -> dict:
        """rt_accum_shutter_info: "static_lights" (no emissive triangle moves: a refit slice skips the light half of the update) and
        "light_rebuilds" (installs since attach that built a light tree)."""
        st, n = C.c_uint32(0), C.c_uint32(0)
        _check(lib().rt_accum_shutter_info(self._h, C.byref(st), C.byref(n)))
        return {"static_lights": bool(st.value), "light_rebuilds": int(n.value)}

    def attach_flow(self, key0=None, key1=None, sensor1=None, reserved=None) -> None:
        """rt_accum_attach_flow (include/rt_abi.h states the rule): keep, per pixel, the motion vectors of its samples: the displacement in
        pixels, from key 0 to key 1, of the surface point each primary ray sees, as the mean over the samples and as the nearest sample's.
        `key0` is the geometry the scene holds now, `key1` the same triangles at the other time: each a scenegen.Scene, a LoadedScene or an
        arrays dict as update_geometry takes them (only the positions are read), a (n, 3, 3) float32 array, or a contiguous float32 torch
        CUDA tensor of the positions (or a dict holding one under "positions"); both keys of one kind. Both None: no triangle moves, the flow
        is the camera's alone. `sensor1`: the view at key 1, a Sensor of the accumulator's kind (None: the view does not move). Once, before
        the first render; not together with a shutter."""
        d = RtFlowDesc()
        for i, r in enumerate(reserved or ()):
            d.reserved[i] = int(r)
        keep = []
        if (key0 is None) != (key1 is None):
            raise ValueError("attach_flow: give both geometry keys or neither")
        if key0 is not None:
            ptrs, counts, on_device = [], set(), None
            for key in (key0, key1):
                if isinstance(key, dict) and hasattr(key.get("positions"), "data_ptr"):
                    key = key["positions"]
                dev_key = hasattr(key, "data_ptr")
                if on_device is not None and dev_key != on_device:
                    raise ValueError("attach_flow: one key is on the device and the other is not")
                on_device = dev_key
                if dev_key:
                    import torch

                    if not key.is_cuda or not key.is_contiguous() or key.dtype != torch.float32:
                        raise TypeError("attach_flow: a device key must be a contiguous float32 torch CUDA tensor")
                    torch.cuda.current_stream(key.device).synchronize()  # the idle precondition
                    ptrs.append(key.data_ptr() if key.numel() else 0)
                    counts.add(key.numel() // 9)
                else:
                    pos = np.ascontiguousarray(key, dtype=np.float32).reshape(-1) if isinstance(key, np.ndarray) else geometry_arrays(key)["positions"]
                    keep.append(pos)
                    ptrs.append(pos.ctypes.data if pos.size else 0)
                    counts.add(pos.size // 9)
            if len(counts) != 1:
                raise ValueError(f"attach_flow: the keys hold different triangle counts {sorted(counts)}")
            d.n_triangles = counts.pop()
            d.flags = RT_FLAG_DEVICE_FB if on_device else 0
            d.positions[0], d.positions[1] = ptrs
        if sensor1 is not None:
            rec = make_sensors([sensor1])
            keep.append(rec)
            d.sensor1 = C.cast(rec, C.POINTER(RtSensor))
        _check(lib().rt_accum_attach_flow(self._h, C.byref(d)))

    def read_flow(self) -> dict:
        """The raw flow state (rt_accum_read_flow): "flow_sum" (H, W, 2) float32, the sum of (dx, dy) over each pixel's valid samples; "valid"
        (H, W) uint32, their number; "near_flow" (H, W, 2) and "near_t" (H, W) float32, the flow and the distance of the nearest valid
        sample. Needs attach_flow."""
        return self._state(lambda *p: lib().rt_accum_read_flow(self._h, *p), flow_sum=(np.float32, 2), valid=(np.uint32,), near_flow=(np.float32, 2), near_t=(np.float32,))

    def flow(self, mode: str = "mean", device_out=None):
        """rt_accum_resolve_flow: (flow (H, W, 2) float32, in pixels, x to the right and y down; mask (H, W) float32, the share of the pixel's
        samples that have a flow). `mode`: "mean" over the valid samples, or "nearest": the flow of the sample nearest to the camera, which
        does not mix two surfaces at an edge. (0, 0) where no sample is valid. `device_out`: a pair of device pointers (flow, mask; either may
        be None or 0) that receive them in HBM (RT_FLAG_DEVICE_FB); then (None, None) is returned."""
        modes = {"mean": RT_FLOW_MEAN, "nearest": RT_FLOW_NEAREST}
        m = modes[mode] if isinstance(mode, str) else int(mode)
        if device_out is not None:
            fp, mp = device_out
            _check(lib().rt_accum_resolve_flow(self._h, m, RT_FLAG_DEVICE_FB, C.c_void_p(fp or None), C.c_void_p(mp or None)))
            return None, None
        flow, mask = self._zeros(np.float32, 2), self._zeros(np.float32)
        _check(lib().rt_accum_resolve_flow(self._h, m, 0, flow.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p)))
        return flow, mask

    def close(self) -> None:
        if self._h:
            lib().rt_accum_destroy(self._h)
            self._h = None
        if self in self._scene._accums:
            self._scene._accums.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bvh_build_host(positions: np.ndarray, subset: Optional[np.ndarray] = None) -> dict:
    """BVH::build (bvh.h:368-393) with the library's host builder, no GPU needed: {root, nodes (n,10) u32, order}."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 9)
    n = pos.shape[0]
    sub = np.arange(n, dtype=np.uint32) if subset is None else np.ascontiguousarray(subset, dtype=np.uint32)
    nodes = np.zeros((2 * len(sub) + 1, 10), dtype=np.uint32)
    order = np.zeros(len(sub), dtype=np.uint32)
    nn, root = C.c_uint32(), C.c_uint32()
    rc = lib().rt_bvh_build_host(fptr(pos), n, u32ptr(sub), len(sub), C.byref(nn), C.byref(root), u32ptr(nodes), u32ptr(order))
    if rc != RT_OK:
        raise RtError(rc, "rt_bvh_build_host")
    return {"root": root.value, "nodes": nodes[: nn.value].copy(), "order": order}


def bvh_wide_build_host(positions: np.ndarray, cost_node: float = 1.0, cost_tri: float = 0.3) -> dict:
    """The production build (RT_BUILD_WIDE) on the host, no GPU needed: {nodes (n,20) u32 WideNode records, order, depth, sah_cost}."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 9)
    n = pos.shape[0]
    nn, depth, cost = C.c_uint32(), C.c_uint32(), C.c_double()
    rc = lib().rt_bvh_wide_build_host(fptr(pos), n, cost_node, cost_tri, C.byref(nn), C.byref(depth), C.byref(cost), None, 0, None)
    if rc != RT_OK:
        raise RtError(rc, "rt_bvh_wide_build_host")
    nodes = np.zeros((nn.value, 20), dtype=np.uint32)
    order = np.zeros(n, dtype=np.uint32)
    rc = lib().rt_bvh_wide_build_host(fptr(pos), n, cost_node, cost_tri, C.byref(nn), C.byref(depth), C.byref(cost), u32ptr(nodes), nn.value, u32ptr(order))
    if rc != RT_OK:
        raise RtError(rc, "rt_bvh_wide_build_host")
    return {"nodes": nodes, "order": order, "depth": depth.value, "sah_cost": cost.value}


def bvh_wide_refit_host(nodes: np.ndarray, order: np.ndarray, positions: np.ndarray) -> np.ndarray:
    """rt_bvh_wide_refit_host: (n, 20) u32 WideNode records (of bvh_wide_build_host or DeviceScene.bvh_wide_dump) refitted to new
    positions, no GPU needed: the CPU model of update_geometry(refit=True). order[k]: original triangle of triangle record k. Returns a copy."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 9)
    out = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 20).copy()
    order = np.ascontiguousarray(order, dtype=np.uint32)
    rc = lib().rt_bvh_wide_refit_host(fptr(pos), pos.shape[0], u32ptr(order), len(order), u32ptr(out), out.shape[0])
    if rc != RT_OK:
        raise RtError(rc, "rt_bvh_wide_refit_host")
    return out


def tonemap(fb: np.ndarray) -> np.ndarray:
    """Image::set_pixel's convert_color (image.h:40-42, 79-82) over a whole linear framebuffer -> (H,W,3) u8."""
    fb = np.ascontiguousarray(fb, dtype=np.float32)
    out = np.zeros(fb.shape, dtype=np.uint8)
    lib().rt_tonemap_rgb8(fptr(fb), fb.size // 3, u8ptr(out))
    return out


def film_table():
    """(thr[256] float32, special[3] uint32): the verified gamma + quantise thresholds the device film searches."""
    thr = np.zeros(256, dtype=np.float32)
    special = np.zeros(3, dtype=np.uint32)
    _check(lib().rt_film_table(fptr(thr), u32ptr(special)))
    return thr, special


def write_ppm(path: str, rgb8: np.ndarray) -> None:
    """Image::write (image.h:34-38)."""
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w, _ = rgb8.shape
    _check(lib().rt_write_ppm(os.fsencode(path), w, h, u8ptr(rgb8)))


def image_decode(path: str) -> np.ndarray:
    """Texture::load_img (geometry.h:584-598) for PNG and JPEG files: (H, W, 4) uint8, the bytes stb_image returns."""
    w, h = C.c_uint32(), C.c_uint32()
    p = c_u8_p()
    _check(lib().rt_image_decode_file(os.fsencode(path), C.byref(w), C.byref(h), C.byref(p)))
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy()
    finally:
        lib().rt_free(p)


def load_hdr(path: str) -> np.ndarray:
    """A picture as radiance for DeviceScene.set_environment: (H, W, 3) float32. A Radiance .hdr gives its values exactly (mantissa *
    2^(e - 136), nothing clipped); a PNG or JPEG its 8-bit texels decoded with the gamma an environment lookup applies."""
    w, h = C.c_uint32(), C.c_uint32()
    p = c_float_p()
    _check(lib().rt_image_decode_radiance(os.fsencode(path), C.byref(w), C.byref(h), C.byref(p)))
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    finally:
        lib().rt_free(p)


def png_decode(path: str) -> np.ndarray:
    w, h = C.c_uint32(), C.c_uint32()
    p = c_u8_p()
    _check(lib().rt_png_decode_file(os.fsencode(path), C.byref(w), C.byref(h), C.byref(p)))
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy()
    finally:
        lib().rt_free(p)


__all__ = [
    "DeviceScene",
    "LoadedScene",
    "RT_ALL_DEVICES",
    "RT_RNG_DEVICE",
    "RT_RNG_REFERENCE",
    "RtError",
    "device_count",
    "lib",
    "parse_gltf_scene",
    "parse_scene_txt",
    "load_scene",
    "make_views",
    "make_sensors",
    "Sensor",
    "RtSensor",
    "RT_LIGHT_GROUP_MAX",
    "RT_LIGHT_GROUP_NONE",
    "pack_rays",
    "rays",
    "RAY_DTYPE",
    "RtRay",
    "pack_bake_points",
    "BAKE_POINT_DTYPE",
    "RtBakePoint",
    "RtBake",
    "RT_BAKE_IRRADIANCE",
    "RT_BAKE_SH9",
    "load_hdr",
    "png_decode",
    "scenegen",
    "tonemap",
    "write_ppm",
]
