"""Test geometries for rt_update_geometry (a plain module next to the tests, imported like conftest's helpers).

Every deformation returns a copy of the scene (dataclasses.replace) with float32 positions; L is the scene's largest extent."""
import dataclasses

import numpy as np

DEFORMATIONS = ("wave", "scatter", "rescale", "flat", "point")
TINY_SIZES = (0, 1, 2, 3, 4, 8, 9, 10, 17, 40)
TOPOLOGY_WORDS = (4, 5, 6)  # child_base, tri_base, tri_mask of a WideNode record; imask is byte 15


# One ulp off the scene's origin grid: the grid then has a cell to measure (hi - base > 0). A point ON the grid has no extent at all, and
# rt_create refuses such a scene for RT_BUILD_WIDE (exponent range), so rt_update_geometry does too: POINT_ON_GRID, a refusal case.
POINT_ON_GRID = np.array([1.5, -2.25, 0.75], dtype=np.float32)
POINT = np.nextafter(POINT_ON_GRID, np.float32(np.inf)).astype(np.float32)


def extent(pos):
    v = np.asarray(pos, dtype=np.float32).reshape(-1, 3)
    return np.float32((v.max(axis=0) - v.min(axis=0)).max()) if len(v) else np.float32(1.0)


def deform_positions(pos, kind, seed=0):
    """(n, 3, 3) float32 positions -> the deformed copy."""
    p = np.asarray(pos, dtype=np.float32).reshape(-1, 3, 3)
    L = extent(p)
    if kind == "wave":  # per vertex: shared vertices stay shared
        v = p.reshape(-1, 3)
        d = np.stack([np.sin(np.float32(7) * v[:, 1] / L), np.sin(np.float32(5) * v[:, 2] / L), np.sin(np.float32(3) * v[:, 0] / L)], axis=1)
        return (v + np.float32(0.05) * L * d.astype(np.float32)).astype(np.float32).reshape(-1, 3, 3)
    if kind == "scatter":  # every triangle by its own offset: the worst case for a stale topology
        off = np.random.default_rng(seed).uniform(-0.5, 0.5, size=(len(p), 1, 3)).astype(np.float32) * L
        return (p + off).astype(np.float32)
    if kind == "rescale":  # grid base, g and e_base all change
        return (p * np.float32(1024.0) + np.array([3000.0, -2000.0, 500.0], dtype=np.float32)).astype(np.float32)
    if kind == "flat":
        q = p.copy()
        q[:, :, 0] = np.float32(0.375) * L
        return q
    if kind == "point":  # zero extent: the exponents clamp to the scene's base
        q = np.empty_like(p)
        q[:] = POINT
        return q
    raise ValueError(kind)


def deform(sc, kind, seed=0):
    return dataclasses.replace(sc, positions=deform_positions(sc.positions, kind, seed))


def emissive_materials(sc):
    return np.array([bool((m.emission_f32() != 0).any()) for m in sc.materials])


def relight(sc, off=False):
    """material_ids changed so that the emissive set changes: every light becomes a plain triangle and (unless `off`) as many other
    triangles take over the emissive materials. A scene without an emissive material gets its ids rotated instead."""
    em = emissive_materials(sc)
    ids = np.asarray(sc.material_ids, dtype=np.uint32).copy()
    if not em.any() or em.all():
        return dataclasses.replace(sc, material_ids=np.roll(ids, 7).astype(np.uint32))
    plain = int(np.flatnonzero(~em)[0])
    lights = np.flatnonzero(em[ids])
    others = np.flatnonzero(~em[ids])
    new = ids.copy()
    new[lights] = plain
    if not off:
        take = others[:: max(1, len(others) // max(1, len(lights)))][: len(lights)]
        new[take] = ids[lights[: len(take)]]
    return dataclasses.replace(sc, material_ids=new.astype(np.uint32))


def tiny_positions(n, seed=3):
    return np.random.default_rng(seed + n).uniform(-1, 1, size=(n, 3, 3)).astype(np.float32)


def topology(nodes):
    """The words of (n, 20) u32 WideNode records a refit must not touch: imask, child_base, tri_base, tri_mask."""
    nodes = np.asarray(nodes, dtype=np.uint32).reshape(-1, 20)
    return np.concatenate([(nodes[:, 3:4] >> 24), nodes[:, list(TOPOLOGY_WORDS)]], axis=1)


def tri_records(positions, order):
    """(a, b - a, c - a) of positions[order] as float32 bit patterns: words 0..8 of the DevTri records of a tree in that order."""
    p = np.asarray(positions, dtype=np.float32).reshape(-1, 3, 3)[np.asarray(order, dtype=np.int64)]
    rec = np.concatenate([p[:, 0], (p[:, 1] - p[:, 0]).astype(np.float32), (p[:, 2] - p[:, 0]).astype(np.float32)], axis=1).astype(np.float32)
    return rec.view(np.uint32)
