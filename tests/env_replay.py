"""The environment rule of include/rt_abi.h (rt_set_environment) restated in numpy: the weights, the tables, pdf, the cell of a direction and the
sampler. The CPU model the GPU's tables and probes are held to (tests/test_gpu_environment.py), itself checked by tests/test_env_replay.py.

float64 where the rule says double, float32 elsewhere: every float32 array meets only np.float32 operands, so each statement rounds once, as
the device's does (-ffp-contract=off). The band factors use math.cos, the host libm's cos the library itself calls. Two things are NOT
restated bit for bit and are only used away from cell edges: rt_bg_uv (the direction's (u, v) is evaluated in float64 here) and the sampler's
sinf / cosf (numpy's, within an ulp of the restated glibc ones)."""
import math

import numpy as np

f32 = np.float32
PI_F = f32(3.14159265358979323846)
SCAN_CHUNKS = 256


def bg_uv64(dirs):
    """rt_bg_uv in float64: u = 0.5 + atan2(z, x) / (2 pi), v = 0.5 - asin(y) / pi. NaN where |y| > 1, as on the device."""
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        u = 0.5 + 0.5 * np.arctan2(d[:, 2], d[:, 0]) / np.pi
        v = 0.5 - np.arcsin(d[:, 1]) / np.pi
    return u, v


def footprint64(u, v, W, H):
    """Texture::sample's addressing in float64: (x0, y0, x1, y1, dx, dy). wrap_repeat maps 1.0 to 0."""
    tx = np.mod(np.mod(u, 1.0) + 1.0, 1.0) * W
    ty = np.mod(np.mod(v, 1.0) + 1.0, 1.0) * H
    x0 = np.minimum(np.floor(tx).astype(np.int64), W - 1)
    y0 = np.minimum(np.floor(ty).astype(np.int64), H - 1)
    return x0, y0, (x0 + 1) % W, (y0 + 1) % H, tx - x0, ty - y0


def radiance64(tex, bg, dirs):
    """Le(dir) = bg * bilinear(tex) in float64, and the footprint it used. A 1x1 map returns its texel."""
    tex = np.asarray(tex, dtype=np.float64)
    H, W = tex.shape[:2]
    bg = np.asarray(bg, dtype=np.float64)
    u, v = bg_uv64(dirs)
    ok = np.isfinite(u) & np.isfinite(v)
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    x0, y0, x1, y1, dx, dy = footprint64(u, v, W, H)
    if W * H == 1:
        return np.broadcast_to(bg * tex[0, 0], (len(u), 3)).copy(), ok, (x0, y0, x1, y1, dx, dy)
    dx3, dy3 = dx[:, None], dy[:, None]
    c = (1 - dx3) * ((1 - dy3) * tex[y0, x0] + dy3 * tex[y1, x0]) + dx3 * ((1 - dy3) * tex[y0, x1] + dy3 * tex[y1, x1])
    return bg * c, ok, (x0, y0, x1, y1, dx, dy)


def luminance32(tex, bg):
    tex = np.asarray(tex, dtype=f32)
    bg = np.asarray(bg, dtype=f32)
    r, g, b = bg[0] * tex[..., 0], bg[1] * tex[..., 1], bg[2] * tex[..., 2]
    return (f32(0.2126) * r + f32(0.7152) * g) + f32(0.0722) * b


def band_factors(W, H):
    """c_i = cos(pi i / H) and Omega_i = (2 pi / W)(c_i - c_(i+1)), double, as rt_env_host.cpp computes them."""
    pi = 3.14159265358979323846
    edge = np.array([1.0 if i == 0 else -1.0 if i == H else math.cos(pi * float(i) / float(H)) for i in range(H + 1)], dtype=np.float64)
    omega = np.array([(2.0 * pi / float(W)) * (edge[i] - edge[i + 1]) for i in range(H)], dtype=np.float64)
    return edge, omega


def weights(tex, bg):
    """M_ij (float32: the largest luminance over the cell's bilinear footprint, at least 0) and w_ij = (double)M_ij * Omega_i."""
    H, W = np.asarray(tex).shape[:2]
    lum = luminance32(tex, bg)
    down, right = np.roll(lum, -1, axis=0), np.roll(lum, -1, axis=1)
    M = np.maximum(np.maximum(np.maximum(np.maximum(f32(0), lum), down), right), np.roll(down, -1, axis=1)).astype(f32)
    _, omega = band_factors(W, H)
    return M, M.astype(np.float64) * omega[:, None]


def prefix(a):
    """The rule's prefix sums over the last axis: 256 chunks of C = ceil(n / 256) elements, each summed left to right, the chunk totals summed
    left to right, P_k = B_c + L_k. np.cumsum adds strictly in order."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[-1]
    C = -(-n // SCAN_CHUNKS)
    pad = np.zeros(a.shape[:-1] + (SCAN_CHUNKS * C - n,), dtype=np.float64)
    L = np.cumsum(np.concatenate([a, pad], axis=-1).reshape(a.shape[:-1] + (SCAN_CHUNKS, C)), axis=-1)
    tot = np.cumsum(L[..., -1], axis=-1)
    B = np.concatenate([np.zeros(a.shape[:-1] + (1,)), tot[..., :-1]], axis=-1)
    P = (B[..., None] + L).reshape(a.shape[:-1] + (SCAN_CHUNKS * C,))[..., :n]
    return P, tot[..., -1]


def cdf32(a):
    """cdf[0] = 0, cdf[k + 1] = (float)(P_k / P_(n-1)), cdf[n] = 1; a sequence of total 0 gets (float)(k + 1) / (float)n. Returns (cdf, total)."""
    P, total = prefix(a)
    n = P.shape[-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (P / total[..., None]).astype(f32)
    uniform = (np.arange(1, n + 1, dtype=np.uint32).astype(f32) / f32(n)).astype(f32)
    c = np.where((total > 0.0)[..., None], c, uniform)
    c[..., -1] = f32(1)
    return np.concatenate([np.zeros(P.shape[:-1] + (1,), dtype=f32), c], axis=-1).astype(f32), total


class Tables:
    """The float tables of a map: rows (H, W + 1), marg (H + 1,), the float edges c (H + 1,) and cell solid angles omega (H,); p (H, W) as the
    rule defines it from the stored tables. `ok` is False when every weight is zero: no distribution."""

    def __init__(self, tex, bg=(1.0, 1.0, 1.0)):
        tex = np.asarray(tex, dtype=f32)
        self.H, self.W = tex.shape[:2]
        self.M, self.w = weights(tex, bg)
        self.rows, row_total = cdf32(self.w)
        self.marg, total = cdf32(row_total)
        self.ok = bool(total > 0.0)
        edge, omega = band_factors(self.W, self.H)
        self.c, self.omega = edge.astype(f32), omega.astype(f32)
        self.p = ((self.marg[1:] - self.marg[:-1])[:, None] * (self.rows[:, 1:] - self.rows[:, :-1])).astype(f32)
        self.pdf_cells = (self.p / self.omega[:, None]).astype(f32)


def cell_of(dirs, W, H):
    """(i, j) of a direction from float64 (u, v), and its distance to the nearest cell edge in texels (the device's float (u, v) can name the
    neighbour within ~1e-6 texels of an edge)."""
    u, v = bg_uv64(dirs)
    x0, y0, _, _, dx, dy = footprint64(u, v, W, H)
    return y0, x0, np.minimum(np.minimum(dx, 1 - dx), np.minimum(dy, 1 - dy))


def select(t, xi):
    """The cell the sampler picks for (n, 4) uniforms: the last i with marg[i] <= x0, the last j with row_i[j] <= x1."""
    xi = np.asarray(xi, dtype=f32).reshape(-1, 4)
    i = np.searchsorted(t.marg, xi[:, 0], side="right") - 1
    i = np.minimum(i, t.H - 1)
    j = np.empty_like(i)
    for r in np.unique(i):
        m = i == r
        j[m] = np.searchsorted(t.rows[r], xi[m, 1], side="right") - 1
    return i, np.minimum(j, t.W - 1)


def sample(t, xi):
    """The sampler's direction, float32 statement by statement (sinf / cosf: numpy's)."""
    xi = np.asarray(xi, dtype=f32).reshape(-1, 4)
    i, j = select(t, xi)
    u = (j.astype(f32) + xi[:, 2]) / f32(t.W)
    ct, cb = t.c[i], t.c[i + 1]
    dy = ct - xi[:, 3] * (ct - cb)
    r = np.sqrt(np.maximum(f32(0), f32(1) - dy * dy)).astype(f32)
    a = ((f32(2) * PI_F) * u).astype(f32)
    s, c = np.sin(a).astype(f32), np.cos(a).astype(f32)
    return np.stack([-(r * c), dy, -(r * s)], axis=1).astype(f32), i, j


def cell_centres(W, H):
    """One direction per cell, in solid-angle terms its middle: u = (j + 0.5) / W, cos(theta) halfway between the row's edges. (H * W, 3) float64."""
    edge, _ = band_factors(W, H)
    cy = 0.5 * (edge[:-1] + edge[1:])
    phi = 2.0 * np.pi * (np.arange(W) + 0.5) / W
    r = np.sqrt(1.0 - cy * cy)
    return np.stack([-(r[:, None] * np.cos(phi)[None, :]), np.broadcast_to(cy[:, None], (H, W)), -(r[:, None] * np.sin(phi)[None, :])], axis=2).reshape(-1, 3)


def histogram_ok(i, j, p, n):
    """Every cell's count within 6 sqrt(p (1 - p) / N) + 1 / N of p_ij. Returns (ok, worst excess over the bound, as a multiple of the bound)."""
    H, W = p.shape
    freq = np.bincount(i * W + j, minlength=H * W).reshape(H, W) / float(n)
    p = p.astype(np.float64)
    bound = 6.0 * np.sqrt(p * (1.0 - p) / n) + 1.0 / n
    return bool((np.abs(freq - p) <= bound).all()), float((np.abs(freq - p) / bound).max())


def sky(W=32, H=16, sun=1000.0):
    """A dim gradient sky with a 2 x 2 texel sun of ~`sun`, float32 (H, W, 3)."""
    y = np.linspace(0.0, 1.0, H)[:, None]
    x = np.linspace(0.0, 1.0, W)[None, :]
    base = 0.05 + 0.25 * (1.0 - y) + 0.0 * x
    tex = np.stack([0.6 * base, 0.8 * base, 1.0 * base], axis=2)
    tex[H // 4:H // 4 + 2, (5 * W) // 8:(5 * W) // 8 + 2] = (sun, 0.9 * sun, 0.7 * sun)
    return tex.astype(f32)
