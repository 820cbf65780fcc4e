"""Cameras as the library takes them: rt_view and rt_sensor records of scenegen.Camera and Sensor objects."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import scenegen
from ._ctypes_abi import (RT_SENSOR_EQUIRECT, RT_SENSOR_FISHEYE, RT_SENSOR_ORTHOGRAPHIC, RT_SENSOR_PINHOLE, RT_SENSOR_THIN_LENS, RtCamera, RtSensor,
                          RtView)


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
