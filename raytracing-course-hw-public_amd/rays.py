"""Ray generators for DeviceScene.render_rays (rt_render_rays): sensor models the library has no camera for, in plain numpy.

Every generator returns W x H x spp packed rays (RAY_DTYPE records, include/rt_abi.h rt_ray) in pixel-major order, the spp rays of a pixel
next to each other, with stream = pixel index (row-major, y down) and first_sample = the ray's index within its pixel. Rendered with
samples=1 and rays_per_output=spp they give one output per pixel: `out.reshape(H, W, 3)`.

Sub-pixel jitter (and the lens samples of thin_lens) comes from numpy's default_rng(seed), in float64 rounded to float32. These generators
are NOT bit-compatible with the reference's gen_ray (raytracer.h:527-538), which draws its jitter from the path's own stream in float32:
`pinhole` is the same camera model as rt_render's, not the same image. The exact path (rt_render's bits from rt_render_rays) goes through
the oracle's logged primary rays (tests/test_gpu_render_rays.py).
"""
from __future__ import annotations

import numpy as np

from ._ctypes_abi import RAY_DTYPE


def _f64(v):
    return np.asarray(v, dtype=np.float64).reshape(3)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _screen(width: int, height: int, spp: int, seed: int, jitter: bool):
    """Continuous pixel coordinates (u, v) in [0, W) x [0, H) of every (pixel, sample), each of shape (H * W * spp,), and the generator."""
    width, height, spp = int(width), int(height), int(spp)
    if width < 1 or height < 1 or spp < 1:
        raise ValueError("width, height and spp must be >= 1")
    rng = np.random.default_rng(seed)
    n = width * height * spp
    pix = np.repeat(np.arange(width * height, dtype=np.int64), spp)
    off = rng.random((n, 2)) if jitter else np.full((n, 2), 0.5)
    return (pix % width) + off[:, 0], (pix // width) + off[:, 1], rng


def _pack(origin, direction, width: int, height: int, spp: int) -> np.ndarray:
    n = int(width) * int(height) * int(spp)
    out = np.zeros(n, dtype=RAY_DTYPE)
    out["origin"] = np.broadcast_to(np.asarray(origin, dtype=np.float64), (n, 3)).astype(np.float32)
    out["dir"] = np.broadcast_to(np.asarray(direction, dtype=np.float64), (n, 3)).astype(np.float32)
    idx = np.arange(n, dtype=np.int64)
    out["stream"] = (idx // spp).astype(np.uint32)
    out["first_sample"] = (idx % spp).astype(np.uint32)
    return out


def _camera_dirs(camera, width, height, u, v):
    """gen_ray's screen point for continuous pixel coordinates: sx * right - sy * up + forward (not normalised)."""
    tan_x = np.tan(float(camera.fov_x) / 2)
    tan_y = tan_x * height / width  # = tan(fov_y / 2) with fov_y = 2 atan(tan(fov_x / 2) * H / W) (scene.h:69-71)
    sx = (2 * u / width - 1) * tan_x
    sy = (2 * v / height - 1) * tan_y
    return sx[:, None] * _f64(camera.right) - sy[:, None] * _f64(camera.up) + _f64(camera.forward)


def pinhole(camera, width: int, height: int, spp: int = 1, seed: int = 0, jitter: bool = True) -> np.ndarray:
    """The pinhole camera of rt_render (a scenegen.Camera, or anything with position / right / up / forward / fov_x): unit directions
    through jittered points of each pixel."""
    u, v, _ = _screen(width, height, spp, seed, jitter)
    return _pack(_f64(camera.position), _unit(_camera_dirs(camera, width, height, u, v)), width, height, spp)


def equirect(position, width: int, height: int, spp: int = 1, seed: int = 0, jitter: bool = True, forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """A full-sphere latitude-longitude panorama from `position`: column -> azimuth in [-pi, pi) around `up` (0 at `forward`, growing to the
    right), row -> elevation from +pi/2 (top) to -pi/2."""
    u, v, _ = _screen(width, height, spp, seed, jitter)
    up = _unit(_f64(up))
    fwd = _f64(forward)
    fwd = _unit(fwd - up * np.dot(fwd, up))
    right = np.cross(fwd, up)
    az = (u / width - 0.5) * 2 * np.pi
    el = (0.5 - v / height) * np.pi
    d = (np.cos(el) * np.sin(az))[:, None] * right + np.sin(el)[:, None] * up + (np.cos(el) * np.cos(az))[:, None] * fwd
    return _pack(_f64(position), _unit(d), width, height, spp)


def orthographic(position, right, up, forward, half_width: float, width: int, height: int, spp: int = 1, seed: int = 0, jitter: bool = True) -> np.ndarray:
    """Parallel rays along `forward` from a film plane centred at `position`, spanned by `right` and `up` (normalised here), 2 * half_width
    wide and 2 * half_width * H / W high."""
    u, v, _ = _screen(width, height, spp, seed, jitter)
    r, w, f = _unit(_f64(right)), _unit(_f64(up)), _unit(_f64(forward))
    sx = (2 * u / width - 1) * float(half_width)
    sy = (2 * v / height - 1) * float(half_width) * height / width
    return _pack(_f64(position) + sx[:, None] * r - sy[:, None] * w, f, width, height, spp)


def thin_lens(camera, aperture: float, focus: float, width: int, height: int, spp: int = 1, seed: int = 0, jitter: bool = True) -> np.ndarray:
    """The pinhole camera with a lens of radius `aperture` focused at distance `focus` along `forward`: each ray starts at a uniform point of
    the lens disc (in the right / up plane) and passes through the point where the pinhole ray meets the focal plane."""
    u, v, rng = _screen(width, height, spp, seed, jitter)
    d = _camera_dirs(camera, width, height, u, v)  # forward component 1: the focal plane is reached at focus * d
    target = _f64(camera.position) + float(focus) * d
    rad = float(aperture) * np.sqrt(rng.random(len(u)))
    phi = 2 * np.pi * rng.random(len(u))
    origin = _f64(camera.position) + (rad * np.cos(phi))[:, None] * _f64(camera.right) + (rad * np.sin(phi))[:, None] * _f64(camera.up)
    return _pack(origin, _unit(target - origin), width, height, spp)


__all__ = ["pinhole", "equirect", "orthographic", "thin_lens"]
