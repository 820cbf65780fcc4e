"""What a call reads: packed rt_ray / rt_bake_point records, and the scene descriptor with its five per-triangle arrays."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import scenegen
from ._ctypes_abi import BAKE_POINT_DTYPE, RAY_DTYPE, DescHolder, RtBakePoint, RtRay, RtSceneDesc
from ._loaded import LoadedScene


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


def _as_desc(scene) -> tuple[RtSceneDesc, object]:
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
