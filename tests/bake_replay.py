"""The bake rule of include/rt_abi.h (rt_bake, rt_bake_rays, rt_lightmap_points) restated in numpy float32, one operation per statement: the
CPU model the GPU's bake rays, folds and light-map points are held to bit for bit (tests/test_gpu_bake.py, tests/test_gpu_lightmap.py) and
that is itself anchored to an independent float64 evaluation (tests/test_bake_replay.py).

Every array is float32 and every scalar operand an np.float32, so each statement rounds once, as the device's statement does
(-ffp-contract=off). The random draws come from oracle.xoshiro_sequence mapped through uniform_real's expression (rt_devspec.h:
canonical * (b - a) + a), sines and cosines from oracle.sincos (the restatement of rt_devspec.h the device evaluates)."""
import importlib

import numpy as np

f32 = np.float32
PI_F = f32(3.14159265358979323846)
DIR_XOR = 0xD6E8FEB86659FD93
IRRADIANCE, SH9 = 0, 1
SH_C = (f32(0.282094792), f32(0.488602512), f32(1.092548431), f32(0.315391565), f32(0.546274215))


def _abi():
    return importlib.import_module("raytracing-course-hw-public_amd._ctypes_abi")


def uniform_real(c, a, b):
    """uniform_real(rng, a, b) of canonical draws c: c * (b - a) + a"""
    w = f32(f32(b) - f32(a))
    r = c * w
    return (r + f32(a)).astype(f32)


def _norm(v):
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    xx = x * x
    yy = y * y
    zz = z * z
    s = xx + yy
    s = s + zz
    ln = np.sqrt(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (v / ln[:, None]).astype(f32)


def sphere_dirs(oracle, seed, stream, smp, with_draws=False):
    """v = sphere_uniform(dg) of the second generator for every (stream[i], smp[i]): (n, 3) float32"""
    n = len(stream)
    c = np.zeros((n, 2), dtype=f32)
    for i in range(n):
        c[i] = oracle.xoshiro_sequence(int(seed) ^ DIR_XOR, int(stream[i]), int(smp[i]), 2)
    z = uniform_real(c[:, 0], -1.0, 1.0)
    zz = z * z
    co = f32(1) - zz
    co = np.where(f32(0) < co, co, f32(0)).astype(f32)  # rmax(0, co) = (0 < co) ? co : 0
    co_z = np.sqrt(co)
    phi = uniform_real(c[:, 1], 0.0, f32(f32(2) * PI_F))
    sn, cs = oracle.sincos(phi)
    v = np.stack([co_z * cs, co_z * sn, z], axis=1).astype(f32)
    assert v.dtype == f32
    return (v, dict(c=c, z=z, phi=phi)) if with_draws else v


def bake_rays(oracle, kind, points, samples, seed=0, offset=0.0, first_sample=0, with_v=False):
    """RAY_DTYPE records of samples [first_sample, first_sample + samples) (mod 2^32) of BAKE_POINT_DTYPE `points`: point-major, stream = the
    point's, first_sample = the sample index."""
    points = np.asarray(points)
    n_pts = len(points)
    n = n_pts * samples
    idx = np.arange(n, dtype=np.int64)
    pt = idx // samples
    smp = ((int(first_sample) + idx % samples) & 0xFFFFFFFF).astype(np.uint32)
    stream = points["stream"][pt].astype(np.uint32)
    v = sphere_dirs(oracle, seed, stream, smp)
    p = points["position"][pt].astype(f32)
    if kind == SH9:
        o, d = p, v
    else:
        nrm = points["normal"][pt].astype(f32)
        d = _norm((nrm + v).astype(f32))
        lift = (f32(offset) * nrm).astype(f32)
        o = (p + lift).astype(f32)
    out = np.zeros(n, dtype=_abi().RAY_DTYPE)
    out["origin"], out["dir"], out["stream"], out["first_sample"] = o, d, stream, smp
    return (out, v) if with_v else out


def sh9(d):
    """Y_k(d) for k < 9: (n, 9) float32"""
    d = np.asarray(d, dtype=f32)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0, c1, c2, c3, c4 = SH_C
    y6 = z * z
    y6 = f32(3.0) * y6
    y6 = y6 - f32(1.0)
    xx = x * x
    yy = y * y
    cols = [np.full(len(d), c0, dtype=f32), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c3 * y6, c2 * (x * z), c4 * (xx - yy)]
    out = np.stack(cols, axis=1).astype(f32)
    assert all(c.dtype == f32 for c in cols)
    return out


def fold_irradiance(per_sample):
    """E = (sum_s L_s / (float)K) * PI_F over (n_points, K, 3) sample values, in sample order from +0.0"""
    a = np.asarray(per_sample, dtype=f32)
    acc = np.zeros((a.shape[0], 3), dtype=f32)
    for s in range(a.shape[1]):
        acc = (acc + a[:, s]).astype(f32)
    acc = (acc / f32(a.shape[1])).astype(f32)
    return (acc * PI_F).astype(f32)


def fold_sh9(per_sample, dirs):
    """C_k = (sum_s (L_s.c * Y_k(d_s)) / (float)K) * (4.0f * PI_F): (n_points, K, 3) values and (n_points, K, 3) directions -> (n_points, 9, 3)"""
    a = np.asarray(per_sample, dtype=f32)
    n, K = a.shape[0], a.shape[1]
    Y = sh9(np.asarray(dirs, dtype=f32).reshape(-1, 3)).reshape(n, K, 9)
    acc = np.zeros((n, 9, 3), dtype=f32)
    for s in range(K):
        term = (a[:, s, None, :] * Y[:, s, :, None]).astype(f32)
        acc = (acc + term).astype(f32)
    acc = (acc / f32(K)).astype(f32)
    return (acc * f32(f32(4.0) * PI_F)).astype(f32)


def lightmap_weights(lm_uv, W, H):
    """The rule's weights of every (triangle, texel) pair: (area (T,), w0, w1, w2 (T, H * W)) in float32"""
    uv = np.asarray(lm_uv, dtype=f32).reshape(-1, 3, 2)
    ax, ay, bx, by, cx_, cy_ = (uv[:, 0, 0, None], uv[:, 0, 1, None], uv[:, 1, 0, None], uv[:, 1, 1, None], uv[:, 2, 0, None], uv[:, 2, 1, None])
    q = np.arange(W * H, dtype=np.int64)
    x = (q % W).astype(f32)
    y = (q // W).astype(f32)
    cx = ((x + f32(0.5)) / f32(W)).astype(f32)[None, :]
    cy = ((y + f32(0.5)) / f32(H)).astype(f32)[None, :]
    with np.errstate(all="ignore"):
        bax, cay, bay, cax = bx - ax, cy_ - ay, by - ay, cx_ - ax
        area = (bax * cay - bay * cax).astype(f32)
        pax, pay = cx - ax, cy - ay
        w1 = ((pax * cay - pay * cax) / area).astype(f32)
        w2 = ((bax * pay - bay * pax) / area).astype(f32)
        w0 = (f32(1.0) - w1).astype(f32)
        w0 = (w0 - w2).astype(f32)
    assert w0.dtype == w1.dtype == w2.dtype == f32
    return area[:, 0], w0, w1, w2


def lightmap_points(positions, normals, lm_uv, W, H):
    """(points (BAKE_POINT_DTYPE), texels (uint32)) of the W x H atlas: every (t, q) pair is tested, the lowest covering t owns q"""
    P = np.asarray(positions, dtype=f32).reshape(-1, 3, 3)
    N = np.asarray(normals, dtype=f32).reshape(-1, 3, 3)
    area, w0, w1, w2 = lightmap_weights(lm_uv, W, H)
    with np.errstate(invalid="ignore"):
        ok = ((area != 0) & np.isfinite(area))[:, None] & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
    owned = ok.any(axis=0)
    texels = np.nonzero(owned)[0].astype(np.uint32)
    t = ok.argmax(axis=0)[texels]  # the first True = the lowest covering triangle
    a, b, c = w0[t, texels][:, None], w1[t, texels][:, None], w2[t, texels][:, None]
    pos = ((a * P[t, 0]).astype(f32) + (b * P[t, 1]).astype(f32)).astype(f32)
    pos = (pos + (c * P[t, 2]).astype(f32)).astype(f32)
    nrm = ((a * N[t, 0]).astype(f32) + (b * N[t, 1]).astype(f32)).astype(f32)
    nrm = _norm((nrm + (c * N[t, 2]).astype(f32)).astype(f32))
    pts = np.zeros(len(texels), dtype=_abi().BAKE_POINT_DTYPE)
    pts["position"], pts["normal"], pts["stream"] = pos, nrm, texels
    return pts, texels
