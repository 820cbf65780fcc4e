"""DeviceScene: a scene and its BVHs in HBM, and every entry point that renders, bakes or queries it (include/rt_abi.h)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from ._accumulator import Accumulator
from ._ctypes_abi import (BAKE_POINT_DTYPE, RAY_DTYPE, RT_ACCUM_FEATURES, RT_BAKE_IRRADIANCE, RT_BAKE_SH9, RT_BUILD_DEVICE_LBVH, RT_BUILD_WIDE, RT_ENV_IMPORTANCE,
                          RT_FLAG_DEVICE_FB, RT_RNG_DEVICE, RT_UPDATE_REBUILD, RT_UPDATE_REFIT, RtBake, RtEnvironment, RtGeometryUpdate, RtSceneDesc, RtStats,
                          fptr, u8ptr, u32ptr)
from ._library import _check, lib
from ._marshal import _deliver, _device_arrays, _device_pair, _params, _render
from ._records import GEOMETRY_ARRAYS, _as_desc, pack_bake_points, pack_rays
from ._sensors import make_sensors, make_views


def _dump(call, *tails) -> tuple:
    """call(&n0, &n1, &word, pointer0, pointer1) of the tree dumps: ask the two sizes, allocate (n_i, *tails[i]) uint32 arrays, ask again.
    Returns (word, array0, array1)."""
    n0, n1, word = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(call(C.byref(n0), C.byref(n1), C.byref(word), None, None))
    a0, a1 = np.zeros((n0.value,) + tails[0], dtype=np.uint32), np.zeros((n1.value,) + tails[1], dtype=np.uint32)
    _check(call(C.byref(n0), C.byref(n1), C.byref(word), u32ptr(a0), u32ptr(a1)))
    return word.value, a0, a1


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
        self._update(lib().rt_update_geometry, desc.n_triangles, refit, [getattr(desc, name) for name, _, _ in GEOMETRY_ARRAYS])

    def _update(self, fn, n_triangles, refit, pointers) -> None:
        """fn(scene, &rt_geometry_update) for the five arrays at `pointers`, in GEOMETRY_ARRAYS' order."""
        u = RtGeometryUpdate(n_triangles, RT_UPDATE_REFIT if refit else RT_UPDATE_REBUILD, *pointers)
        _check(fn(self._h, C.byref(u)))

    def update_geometry_device(self, positions, normals, texcoords, tangents, material_ids, refit: bool = False, n_triangles: Optional[int] = None) -> None:
        """rt_update_geometry_device: update_geometry for arrays that are on this scene's GPU already. Each argument is a contiguous torch
        CUDA tensor (float32; the ids int32 or uint32) of 9 / 9 / 6 / 9 / 1 elements per triangle, or an int device pointer, used with
        `n_triangles`. Normals are required (the geometric-normal default of update_geometry is host code). The tensors are read, not kept
        and not written; torch's current stream on their device is synchronised first, so that they are idle when the library reads them
        on the scene's own stream."""
        given = dict(positions=positions, normals=normals, texcoords=texcoords, tangents=tangents, material_ids=material_ids)
        rows = [(name, given[name], per, ("float32",) if dtype == np.float32 else ("int32", "uint32")) for name, per, dtype in GEOMETRY_ARRAYS]
        ptrs, n = _device_arrays(rows, n_triangles, same_device=True, strict=True, scene_device=self._device)
        typed = [C.cast(C.c_void_p(ptr), C.POINTER(C.c_float if dtype == np.float32 else C.c_uint32)) for (_, _, dtype), ptr in zip(GEOMETRY_ARRAYS, ptrs)]
        self._update(lib().rt_update_geometry_device, int(n), refit, typed)

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
        recs, k = make_sensors(sensors), len(sensors)
        p, keep = _params(width, height, samples, counters=counters, global_best=global_best, tuning=tuning)  # noqa: F841
        fn = lib().rt_render_sensors_rgb8 if rgb8 else lib().rt_render_sensors
        return _render(fn, self._h, p, (recs, k), (k, height, width, 3), np.uint8 if rgb8 else np.float32, device_out)

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
        return _deliver(lambda flags, q: lib().rt_sensor_rays(*args, flags, q), (int(n_pixels) * int(samples),), RAY_DTYPE, device_out)

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
        p, keep = _params(width, height, samples, rng_mode, seed, (shard_index, shard_count, shard_block), counters, megakernel, global_best, tuning)  # noqa: F841
        return _render(lib().rt_render, self._h, p, (), (height, width, 3), np.float32, device_fb, out)

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
        p, keep = _params(width, height, samples, rng_mode, seed, (shard_index, shard_count, shard_block), global_best=global_best, tuning=tuning)  # noqa: F841
        return _render(lib().rt_render_rgb8, self._h, p, (), (height, width, 3), np.uint8, device_rgb8, out)

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
        views, k = make_views(cameras, seeds), len(cameras)
        p, keep = _params(width, height, samples, rng_mode, 0, (shard_index, shard_count, shard_block), counters, megakernel, global_best, tuning)  # noqa: F841
        fn = lib().rt_render_views_rgb8 if rgb8 else lib().rt_render_views
        return _render(fn, self._h, p, (views, k), (k, height, width, 3), np.uint8 if rgb8 else np.float32, device_fb, out)

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
        p, keep = _params(0, 0, int(samples), seed=int(seed), counters=counters, global_best=global_best, tuning=tuning)  # noqa: F841
        fn = lib().rt_render_rays_rgb8 if rgb8 else lib().rt_render_rays
        g = int(rays_per_output)
        if _device_pair("render_rays", "rays", device_rays, n_rays, device_out):
            src, n = C.c_void_p(device_rays), int(n_rays)
        else:
            packed = pack_rays(rays, stream, first_sample, samples=int(samples), rays_per_output=max(1, g))
            src, n = packed.ctypes.data_as(C.c_void_p), len(packed)
        return _render(fn, self._h, p, (src, n, g), (n // max(1, g), 3), np.uint8 if rgb8 else np.float32, device_out)

    def _bake_points(self, who, points, device_points, n_points, device_out):
        """The points of a bake or of its rays as (pointer, count, what keeps them alive): `points` packed, or the device form."""
        if _device_pair(who, "points", device_points, n_points, device_out):
            return C.c_void_p(device_points), int(n_points), None
        packed = pack_bake_points(points)
        return packed.ctypes.data_as(C.c_void_p), len(packed), packed

    def _bake(self, kind, points, samples, seed, offset, first_sample, device_points, n_points, device_out, global_best, counters, tuning):
        p, keep = _params(0, 0, int(samples), seed=int(seed), counters=counters, global_best=global_best, tuning=tuning)  # noqa: F841
        b = RtBake(int(kind), int(first_sample) & 0xFFFFFFFF, float(offset))
        src, n, packed = self._bake_points("bake", points, device_points, n_points, device_out)  # noqa: F841
        return _render(lib().rt_bake, self._h, p, (C.byref(b), src, n), (n,) + ((9, 3) if kind == RT_BAKE_SH9 else (3,)), np.float32, device_out)

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
        src, n, packed = self._bake_points("bake_rays", points, device_points, n_points, device_out)  # noqa: F841
        return _deliver(lambda flags, q: lib().rt_bake_rays(self._h, C.byref(b), int(seed), src, n, int(samples), flags, q), (n * int(samples),), RAY_DTYPE, device_out)

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
            ptrs, n = _device_arrays([("positions", positions, 9, ("float32",)), ("normals", normals, 9, ("float32",)), ("lm_uv", lm_uv, 6, ("float32",))], n_triangles)
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
        root, nodes, tris = _dump(lambda *a: lib().rt_bvh_device_dump(self._h, which, *a), (16,), (12,))
        return {"root": root, "nodes": nodes, "tris": tris}

    def bvh_compact_dump(self) -> np.ndarray:
        """The compact node records of the binary scene tree read back from HBM: (n_inner, 8) u32, in bvh_device_dump(0)'s node order."""
        n = C.c_uint32()
        _check(lib().rt_bvh_compact_dump(self._h, C.byref(n), None))
        out = np.zeros((n.value, 8), dtype=np.uint32)
        _check(lib().rt_bvh_compact_dump(self._h, C.byref(n), u32ptr(out)))
        return out

    def bvh_patch_plane(self, node: int, word: int, value: float) -> None:
        """rt_bvh_patch_plane (test aid): one plane of one node record in HBM, then the compact records derived again."""
        _check(lib().rt_bvh_patch_plane(self._h, node, word, float(value)))

    def second_visits(self) -> int:
        """rt_second_visits: inner-node visits of the last counted call that ran from a compact record."""
        n = C.c_uint64()
        _check(lib().rt_second_visits(self._h, C.byref(n)))
        return n.value

    def bvh_wide_dump(self):
        """The 8-wide scene BVH read back from HBM: {depth, nodes (n,20) u32 (WideNode records), tris (n_tris,12) u32}."""
        depth, nodes, tris = _dump(lambda *a: lib().rt_bvh_wide_dump(self._h, *a), (20,), (12,))
        return {"depth": depth, "nodes": nodes, "tris": tris}

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
        root, nodes, order = _dump(lambda *a: lib().rt_bvh_info(self._h, which, *a), (10,), ())
        return {"root": root, "nodes": nodes, "order": order}
