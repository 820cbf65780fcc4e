"""Accumulator: resumable per-pixel sample sums of one view of a DeviceScene, and their optional layers (include/rt_abi.h rt_accum_*)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from ._ctypes_abi import RT_FLOW_MEAN, RT_FLOW_NEAREST, RtAdaptive, RtStats, fptr, u32ptr
from ._library import _check, lib
from ._marshal import _deliver, _deliver_each, _denoise_desc, _flow_desc, _ids_desc, _light_groups_desc, _params, _shutter_desc
from ._sensors import make_sensors, make_views


class Accumulator:
    """Progressive and adaptive rendering (include/rt_abi.h rt_accum_*): per-pixel sums S, E (even-index samples) and counts n that
    survive between calls. Keeps its DeviceScene alive; DeviceScene.close() closes it first."""

    def __init__(self, scene: DeviceScene, width: int, height: int, camera=None, seed: int = 0, accum_flags: int = 0, sensor=None):  # noqa: F821
        self._scene = scene
        self.width, self.height = int(width), int(height)
        self.id_slots = self.n_light_groups = 1  # K of read_ids(), G of the light-group reads: 1 until attach_ids / attach_light_groups
        self._h = C.c_void_p()
        cam = None
        if camera is not None:
            cam = make_views([camera], 0)[0].camera
        cam_p = C.byref(cam) if cam is not None else None
        if sensor is not None:
            _check(lib().rt_accum_create_sensor(scene._h, self.width, self.height, make_sensors([sensor]), int(accum_flags), C.byref(self._h)))
        elif accum_flags:
            _check(lib().rt_accum_create_ex(scene._h, self.width, self.height, cam_p, int(seed), int(accum_flags), C.byref(self._h)))
        else:
            _check(lib().rt_accum_create(scene._h, self.width, self.height, cam_p, int(seed), C.byref(self._h)))
        scene._accums.append(self)

    def _state(self, call, device_out=None, **arrays):
        """_deliver_each over this accumulator's pixels: name -> an (H, W, *tail) array per `arrays` (name=(dtype, *tail))."""
        return _deliver_each(call, (self.height, self.width), arrays, device_out)

    def _output(self, call, dtype=np.float32, tail=(3,), device_out=None):
        """_deliver over this accumulator's pixels: the one (H, W, *tail) output of call(flags, pointer)."""
        return _deliver(call, (self.height, self.width) + tail, dtype, device_out)

    def render(self, samples: int, global_best: bool = False, counters: bool = False, **tuning) -> dict:
        """rt_accum_render: `samples` more samples for every pixel. `tuning`: as DeviceScene.run_raytracer. Returns the stats dict."""
        p, keep = _params(self.width, self.height, samples, counters=counters, global_best=global_best, tuning=tuning)  # noqa: F841
        st = RtStats()
        _check(lib().rt_accum_render(self._h, C.byref(p), C.byref(st)))
        return st.as_dict()

    def render_adaptive(self, threshold: float, min_samples: int = 16, max_samples: int = 256, step: int = 32, global_best: bool = False,
                        counters: bool = False, **tuning) -> dict:
        """rt_accum_render_adaptive: rounds of `step` samples for the pixels whose 3x3 window holds an error above `threshold`, until none
        does or they reach `max_samples`. Returns the stats dict with "rounds"."""
        p, keep = _params(self.width, self.height, 0, counters=counters, global_best=global_best, tuning=tuning)  # noqa: F841
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
        return self._state(lambda _, *p: lib().rt_accum_read(self._h, *p), sum=(np.float32, 3), even_sum=(np.float32, 3), samples=(np.uint32,), error=(np.float32,))

    def read_features(self) -> dict:
        """The raw first-hit sums (rt_accum_read_features): "albedo_sum" and "normal_sum" (H, W, 3) float32, "depth_sum" (H, W) float32,
        "hits" (H, W) uint32. Needs accumulator(features=True)."""
        return self._state(lambda _, *p: lib().rt_accum_read_features(self._h, *p), albedo_sum=(np.float32, 3), normal_sum=(np.float32, 3), depth_sum=(np.float32,),
                           hits=(np.uint32,))

    def features(self) -> dict:
        """The feature means (rt_accum_resolve_features): "albedo" = AS / n and "normal" = NS / n (not renormalised), (H, W, 3) float32;
        "depth" = ZS / h (0 where no sample hit), (H, W) float32."""
        return self._state(lambda flags, *p: lib().rt_accum_resolve_features(self._h, flags, *p), albedo=(np.float32, 3), normal=(np.float32, 3), depth=(np.float32,))

    def denoise(self, rgb8: bool = False, **opts) -> np.ndarray:
        """rt_accum_denoise: the image filtered by the edge-avoiding a-trous filter that the feature means and the half-buffer noise estimate
        guide; the accumulator is not modified. `opts`: rt_denoise fields by name (iterations, sigma_color, sigma_depth, normal_sharpness,
        flags, reserved) or demodulate=False for RT_DENOISE_NO_DEMODULATE. (H, W, 3) float32, or the device film's uint8 image with `rgb8`."""
        o, _ = _denoise_desc(opts)
        fn = lib().rt_accum_denoise_rgb8 if rgb8 else lib().rt_accum_denoise
        return self._output(lambda flags, p: fn(self._h, C.byref(o), flags, p), np.uint8 if rgb8 else np.float32)

    def attach_ids(self, kind="primitive", slots: int = 4, n_table: Optional[int] = None) -> None:
        """rt_accum_attach_ids: keep, per pixel, a table of `slots` (id, count) pairs of the ids its samples' primary rays hit, first seen first,
        and a count of the samples that found the table full. `kind`: "primitive" (what cast_rays reports), "material", or a table of user
        ids, one per original triangle and then per analytic primitive: a uint32 array (copied), or a device pointer (an int, with `n_table`
        entries; RT_FLAG_DEVICE_FB). Once, before the first render."""
        d, keep = _ids_desc(kind, slots, n_table)  # noqa: F841 (the table is copied during the call)
        _check(lib().rt_accum_attach_ids(self._h, C.byref(d)))
        self.id_slots = int(d.slots) if d.slots else 4

    def read_ids(self) -> dict:
        """The id tables (rt_accum_read_ids): "ids" and "counts" (H, W, K) uint32 in first-seen order (an empty slot reads id 0, count 0),
        "other" (H, W) uint32: the samples no slot was left for. Needs attach_ids."""
        return self._state(lambda _, *p: lib().rt_accum_read_ids(self._h, *p), ids=(np.uint32, self.id_slots), counts=(np.uint32, self.id_slots), other=(np.uint32,))

    def labels(self, device_out=None):
        """rt_accum_resolve_labels: (label (H, W) uint32: the id of each pixel's fullest slot, RT_ID_MISS where n = 0; coverage (H, W) float32:
        that slot's count / n). `device_out`: a pair of device pointers (label, coverage; either may be None or 0) that receive them in HBM
        (RT_FLAG_DEVICE_FB); then (None, None) is returned."""
        return tuple(self._state(lambda flags, *p: lib().rt_accum_resolve_labels(self._h, flags, *p), device_out, label=(np.uint32,), coverage=(np.float32,)).values())

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
        d, keep = _light_groups_desc(material_group, background, n_groups, n_materials)  # noqa: F841 (copied during the call)
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
        d, keep = _shutter_desc(key0, key1, sensor1, open, close, slices, block, refit, reserved)  # noqa: F841 (copied during the call)
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
        d, keep = _flow_desc(key0, key1, sensor1, reserved)  # noqa: F841 (copied during the call)
        _check(lib().rt_accum_attach_flow(self._h, C.byref(d)))

    def read_flow(self) -> dict:
        """The raw flow state (rt_accum_read_flow): "flow_sum" (H, W, 2) float32, the sum of (dx, dy) over each pixel's valid samples; "valid"
        (H, W) uint32, their number; "near_flow" (H, W, 2) and "near_t" (H, W) float32, the flow and the distance of the nearest valid
        sample. Needs attach_flow."""
        return self._state(lambda _, *p: lib().rt_accum_read_flow(self._h, *p), flow_sum=(np.float32, 2), valid=(np.uint32,), near_flow=(np.float32, 2),
                           near_t=(np.float32,))

    def flow(self, mode: str = "mean", device_out=None):
        """rt_accum_resolve_flow: (flow (H, W, 2) float32, in pixels, x to the right and y down; mask (H, W) float32, the share of the pixel's
        samples that have a flow). `mode`: "mean" over the valid samples, or "nearest": the flow of the sample nearest to the camera, which
        does not mix two surfaces at an edge. (0, 0) where no sample is valid. `device_out`: a pair of device pointers (flow, mask; either may
        be None or 0) that receive them in HBM (RT_FLAG_DEVICE_FB); then (None, None) is returned."""
        modes = {"mean": RT_FLOW_MEAN, "nearest": RT_FLOW_NEAREST}
        m = modes[mode] if isinstance(mode, str) else int(mode)
        return tuple(self._state(lambda flags, *p: lib().rt_accum_resolve_flow(self._h, m, flags, *p), device_out, flow=(np.float32, 2), mask=(np.float32,)).values())

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
