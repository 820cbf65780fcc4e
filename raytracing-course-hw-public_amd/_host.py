"""Functions that need no GPU: the host BVH builders, the film, image files in and out."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np

from ._ctypes_abi import RT_OK, c_float_p, c_u8_p, fptr, u8ptr, u32ptr
from ._library import RtError, _check, lib


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


def _ok(rc: int, what: str) -> None:
    if rc != RT_OK:  # the host builders leave no message behind
        raise RtError(rc, what)


def bvh_build_host(positions: np.ndarray, subset: Optional[np.ndarray] = None) -> dict:
    """BVH::build (bvh.h:368-393) with the library's host builder, no GPU needed: {root, nodes (n,10) u32, order}."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 9)
    n = pos.shape[0]
    sub = np.arange(n, dtype=np.uint32) if subset is None else np.ascontiguousarray(subset, dtype=np.uint32)
    nodes = np.zeros((2 * len(sub) + 1, 10), dtype=np.uint32)
    order = np.zeros(len(sub), dtype=np.uint32)
    nn, root = C.c_uint32(), C.c_uint32()
    rc = lib().rt_bvh_build_host(fptr(pos), n, u32ptr(sub), len(sub), C.byref(nn), C.byref(root), u32ptr(nodes), u32ptr(order))
    _ok(rc, "rt_bvh_build_host")
    return {"root": root.value, "nodes": nodes[: nn.value].copy(), "order": order}


def compact_derive_host(nodes: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """rt_compact_derive_host, no GPU needed: the compact records and selector words of DevNode records (n, 16) u32 (DeviceScene.bvh_device_dump,
    or a tree flattened on the host), by the code the device runs. Returns (a copy of the records with word 14 set, compact records (n, 8) u32)."""
    nodes = np.array(nodes, dtype=np.uint32).reshape(-1, 16)
    compact = np.zeros((nodes.shape[0], 8), dtype=np.uint32)
    _ok(lib().rt_compact_derive_host(u32ptr(nodes), nodes.shape[0], u32ptr(compact)), "rt_compact_derive_host")
    return nodes, compact


def bvh_wide_build_host(positions: np.ndarray, cost_node: float = 1.0, cost_tri: float = 0.3) -> dict:
    """The production build (RT_BUILD_WIDE) on the host, no GPU needed: {nodes (n,20) u32 WideNode records, order, depth, sah_cost}."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 9)
    n = pos.shape[0]
    nn, depth, cost = C.c_uint32(), C.c_uint32(), C.c_double()
    rc = lib().rt_bvh_wide_build_host(fptr(pos), n, cost_node, cost_tri, C.byref(nn), C.byref(depth), C.byref(cost), None, 0, None)
    _ok(rc, "rt_bvh_wide_build_host")
    nodes = np.zeros((nn.value, 20), dtype=np.uint32)
    order = np.zeros(n, dtype=np.uint32)
    rc = lib().rt_bvh_wide_build_host(fptr(pos), n, cost_node, cost_tri, C.byref(nn), C.byref(depth), C.byref(cost), u32ptr(nodes), nn.value, u32ptr(order))
    _ok(rc, "rt_bvh_wide_build_host")
    return {"nodes": nodes, "order": order, "depth": depth.value, "sah_cost": cost.value}


def bvh_wide_refit_host(nodes: np.ndarray, order: np.ndarray, positions: np.ndarray) -> np.ndarray:
    """rt_bvh_wide_refit_host: (n, 20) u32 WideNode records (of bvh_wide_build_host or DeviceScene.bvh_wide_dump) refitted to new
    positions, no GPU needed: the CPU model of update_geometry(refit=True). order[k]: original triangle of triangle record k. Returns a copy."""
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 9)
    out = np.ascontiguousarray(nodes, dtype=np.uint32).reshape(-1, 20).copy()
    order = np.ascontiguousarray(order, dtype=np.uint32)
    rc = lib().rt_bvh_wide_refit_host(fptr(pos), pos.shape[0], u32ptr(order), len(order), u32ptr(out), out.shape[0])
    _ok(rc, "rt_bvh_wide_refit_host")
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


def _decode(fn, path, pointer_type, channels) -> np.ndarray:
    """fn(path, &width, &height, &texels): a copy of the (H, W, channels) image the library allocated, which is freed."""
    w, h, p = C.c_uint32(), C.c_uint32(), pointer_type()
    _check(fn(os.fsencode(path), C.byref(w), C.byref(h), C.byref(p)))
    try:
        return np.ctypeslib.as_array(p, shape=(h.value, w.value, channels)).copy()
    finally:
        lib().rt_free(p)


def image_decode(path: str) -> np.ndarray:
    """Texture::load_img (geometry.h:584-598) for PNG and JPEG files: (H, W, 4) uint8, the bytes stb_image returns."""
    return _decode(lib().rt_image_decode_file, path, c_u8_p, 4)


def load_hdr(path: str) -> np.ndarray:
    """A picture as radiance for DeviceScene.set_environment: (H, W, 3) float32. A Radiance .hdr gives its values exactly (mantissa *
    2^(e - 136), nothing clipped); a PNG or JPEG its 8-bit texels decoded with the gamma an environment lookup applies."""
    return _decode(lib().rt_image_decode_radiance, path, c_float_p, 3)


def png_decode(path: str) -> np.ndarray:
    return _decode(lib().rt_png_decode_file, path, c_u8_p, 4)
