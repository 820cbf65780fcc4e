"""The shutter rule of include/rt_abi.h (rt_accum_attach_shutter) in numpy, operation by operation in float32 (a plain module next to the
tests, imported like update_geometry.py): the slice of a sample, the time of a slice, the geometry and the sensor at a time, and the
in-order float32 sums of an accumulator. Nothing here calls the library."""
import dataclasses

import numpy as np

F = np.float32
INTERPOLATED = ("positions", "normals", "tangents")
SENSOR_SCALARS = ("half_width", "lens_radius", "focus_distance")


def bit_reverse(j: int, slices: int) -> int:
    k, bit = 0, 1
    while bit < slices:
        k = (k << 1) | (j & 1)
        j >>= 1
        bit <<= 1
    return k


def slice_of(s: int, slices: int, block: int) -> int:
    """k of sample index s: the bit-reversed (s // B) mod K."""
    return bit_reverse((s // block) % slices, slices)


def slice_time(k: int, slices: int, open=0.0, close=1.0) -> np.float32:
    """t_k = open + (close - open) * (((float)k + 0.5f) / (float)K)."""
    o, c = F(open), F(close)
    return F(o + F(F(c - o) * F(F(F(k) + F(0.5)) / F(slices))))


def runs(n: int, samples: int, slices: int, block: int):
    """The maximal runs (first sample, length, slice) of one slice in [n, n + samples)."""
    out, s, end = [], n, n + samples
    while s < end:
        k, e = slice_of(s, slices, block), s + 1
        while e < end and slice_of(e, slices, block) == k:
            e += 1
        out.append((s, e - s, k))
        s = e
    return out


def blend_raw(x0, x1, t):
    """b = x0 + t * (x1 - x0): three float32 roundings."""
    x0, x1 = np.asarray(x0, dtype=F), np.asarray(x1, dtype=F)
    with np.errstate(over="ignore", invalid="ignore"):
        return (x0 + (F(t) * (x1 - x0).astype(F)).astype(F)).astype(F)


def blend(x0, x1, t):
    """x(t): b held between the keys by comparisons alone."""
    x0, x1 = np.asarray(x0, dtype=F), np.asarray(x1, dtype=F)
    b = blend_raw(x0, x1, t)
    up = x0 <= x1
    lo, hi = np.where(up, x0, x1), np.where(up, x1, x0)
    with np.errstate(invalid="ignore"):
        return np.where(~(b > lo), lo, np.where(~(b < hi), hi, b)).astype(F)


def geometry_at(key0: dict, key1: dict, t) -> dict:
    """The five flat arrays at time t from two dicts of flat arrays: positions, normals and tangents blended, the rest key 0's."""
    out = {name: np.asarray(a).copy() for name, a in key0.items()}
    for name in INTERPOLATED:
        out[name] = blend(key0[name], key1[name], t)
    return out


def _axis(a0, a1, t):
    v = blend_raw(a0, a1, t)
    x, y, z = v
    length = np.sqrt(F(F(F(x * x) + F(y * y)) + F(z * z)))
    return np.array([x / length, y / length, z / length], dtype=F)


def sensor_at(s0, s1, t):
    """The Sensor at time t between two Sensor objects of one kind (s1 None: s0 itself, untouched)."""
    if s1 is None:
        return s0
    c0, c1 = s0.camera, s1.camera
    cam = dataclasses.replace(c0, position=blend_raw(c0.position, c1.position, t), right=_axis(c0.right, c1.right, t), up=_axis(c0.up, c1.up, t),
                              forward=_axis(c0.forward, c1.forward, t), fov_x=float(blend_raw(F(c0.fov_x), F(c1.fov_x), t)))
    scalars = {name: float(blend_raw(F(getattr(s0, name)), F(getattr(s1, name)), t)) for name in SENSOR_SCALARS}
    return dataclasses.replace(s0, camera=cam, **scalars)


def accumulate(sample, n_samples: int, shape):
    """(S, E): the in-order float32 sums over s < n_samples of sample(s) (an array of `shape`), E over even s, from +0."""
    S, E = np.zeros(shape, dtype=F), np.zeros(shape, dtype=F)
    for s in range(n_samples):
        x = np.asarray(sample(s), dtype=F).reshape(shape)
        S = (S + x).astype(F)
        if s % 2 == 0:
            E = (E + x).astype(F)
    return S, E
