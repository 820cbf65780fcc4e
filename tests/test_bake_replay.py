"""The bake replay (tests/bake_replay.py) anchored without a GPU: its directions against a float64 evaluation of the same formulas from the
same draws, its SH basis against orthonormality under a float64 quadrature, its rasteriser against a float64 point-in-triangle test. The GPU
tests hold the device to the replay bit for bit; these hold the replay to the mathematics.

"The same draws" are the rule's two uniform_real draws z and phi, as tests/test_sensor_replay.py starts its float64 evaluation from the
model's uniform_real draws; test_draws_are_uniform_real_of_the_canonical_draws ties them to the generator's canonical output. (From the
canonical draws the rounding of phi alone, half an ulp of a number near 2 pi = 2^-22, reaches 2^-19 in a direction with |n + v| = 0.1.)"""
import numpy as np
import pytest

import bake_replay as br

f32 = np.float32
SEED = 11


@pytest.fixture(scope="module")
def draws(oracle):
    """4096 samples of one stream: the replay's float32 directions v, and what they were made of (canonical draws c, z, phi)"""
    n = 4096
    stream = np.full(n, 5, dtype=np.uint32)
    smp = np.arange(n, dtype=np.uint32)
    v, d = br.sphere_dirs(oracle, SEED, stream, smp, with_draws=True)
    return v, d, stream, smp


def _dirs64(d):
    """sphere_uniform in float64 from the rule's two draws z = uniform_real(dg, -1, 1) and phi = uniform_real(dg, 0, 2 pi), as
    tests/test_sensor_replay.py starts its float64 evaluation from the model's uniform_real draws"""
    z, phi = d["z"].astype(np.float64), d["phi"].astype(np.float64)
    co = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([co * np.cos(phi), co * np.sin(phi), z], axis=1)


def test_draws_are_uniform_real_of_the_canonical_draws(draws):
    _, d, _, _ = draws
    c = d["c"].astype(np.float64)
    assert np.all((c >= 0) & (c < 1))
    # c * 2 - 1 rounds twice at magnitudes <= 2 and <= 1: 2^-24 + 2^-25
    assert np.abs(d["z"] - (2.0 * c[:, 0] - 1.0)).max() <= 2.0 ** -24 + 2.0 ** -25
    # c * (2 PI_F) rounds once at a magnitude < 8 (half an ulp: 2^-22), and 2 PI_F is 2 pi to 1.75e-7 < 2^-22
    assert np.abs(d["phi"] - 2.0 * np.pi * c[:, 1]).max() <= 2.0 ** -21
    assert d["phi"].min() >= 0 and d["phi"].max() <= float(f32(2) * br.PI_F) and np.abs(d["z"]).max() <= 1


def test_directions_agree_with_float64(oracle, draws):
    v, d, stream, smp = draws
    v64 = _dirs64(d)
    assert np.abs(v.astype(np.float64) - v64).max() <= 2.0 ** -20  # SH9: d = v
    nrm = np.array([0.0, 0.6, 0.8], dtype=f32)
    pts = np.zeros(1, dtype=br._abi().BAKE_POINT_DTYPE)
    pts["position"], pts["normal"], pts["stream"] = (1.0, 2.0, 3.0), nrm, 5
    rays = br.bake_rays(oracle, br.IRRADIANCE, pts, len(v), seed=SEED, offset=0.25)
    assert np.array_equal(rays["first_sample"], smp) and np.all(rays["stream"] == 5)
    s64 = nrm.astype(np.float64)[None, :] + v64
    ln = np.linalg.norm(s64, axis=1)
    keep = ln >= 0.1  # below that the normalisation amplifies the rounding of n + v; P(|n + v| < 0.1) = 0.0025
    assert np.count_nonzero(~keep) <= len(v) // 100
    d64 = s64[keep] / ln[keep, None]
    assert np.abs(rays["dir"][keep].astype(np.float64) - d64).max() <= 2.0 ** -20
    # the origin: p + offset * n, exactly representable here
    assert np.array_equal(rays["origin"], np.tile((np.array([1.0, 2.0, 3.0], dtype=f32) + f32(0.25) * nrm).astype(f32), (len(v), 1)))
    # the cosine lobe: E[dot(n, d)] = 2/3, Var = 1/2 - 4/9 = 1/18
    cosv = d64 @ nrm.astype(np.float64)
    sigma = np.sqrt((1.0 / 18.0) / len(cosv))
    assert abs(cosv.mean() - 2.0 / 3.0) <= 6.0 * sigma, (cosv.mean(), sigma)


def test_sample_index_wraps_and_kinds_share_the_generator(oracle):
    pts = np.zeros(2, dtype=br._abi().BAKE_POINT_DTYPE)
    pts["normal"] = (0, 0, 1)
    pts["stream"] = (3, 9)
    a, va = br.bake_rays(oracle, br.IRRADIANCE, pts, 5, seed=SEED, first_sample=2 ** 32 - 3, with_v=True)
    assert list(a["first_sample"][:5]) == [2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1, 0, 1]
    b = br.bake_rays(oracle, br.SH9, pts, 5, seed=SEED, first_sample=2 ** 32 - 3)
    assert np.array_equal(b["dir"].view(np.uint32), va.view(np.uint32))  # SH9's direction is the v IRRADIANCE adds to the normal
    # the direction generator is not the path's: its draws differ from the stream's own first two
    own = oracle.xoshiro_sequence(SEED, 3, 0, 2)
    other = oracle.xoshiro_sequence(SEED ^ br.DIR_XOR, 3, 0, 2)
    assert not np.array_equal(own, other)


def test_sh9_is_orthonormal():
    nz, nphi = 32, 64
    x, w = np.polynomial.legendre.leggauss(nz)  # exact for the degree-4 polynomials in z; uniform phi is exact for the harmonics up to 4 phi
    phi = (np.arange(nphi) + 0.5) * (2.0 * np.pi / nphi)
    Z, PH = np.meshgrid(x, phi, indexing="ij")
    co = np.sqrt(1.0 - Z * Z)
    d = np.stack([co * np.cos(PH), co * np.sin(PH), Z], axis=-1).reshape(-1, 3)
    wt = np.repeat(w, nphi) * (2.0 * np.pi / nphi)
    # the float32 constants, evaluated in float64: the constants carry 9 digits
    c0, c1, c2, c3, c4 = (float(c) for c in br.SH_C)
    X, Y, Zz = d[:, 0], d[:, 1], d[:, 2]
    B = np.stack([np.full(len(d), c0), c1 * Y, c1 * Zz, c1 * X, c2 * X * Y, c2 * Y * Zz, c3 * (3 * Zz * Zz - 1), c2 * X * Zz, c4 * (X * X - Y * Y)], axis=1)
    G = (B * wt[:, None]).T @ B
    assert np.abs(G - np.eye(9)).max() <= 1e-6
    # the replay's float32 basis is that basis
    assert np.abs(br.sh9(d.astype(f32)).astype(np.float64) - B).max() <= 1e-6


def test_folds_are_the_rule_in_order():
    rng = np.random.default_rng(3)
    L = rng.uniform(0, 4, size=(5, 7, 3)).astype(f32)
    E = br.fold_irradiance(L)
    acc = np.zeros(3, dtype=f32)
    for s in range(7):
        acc = (acc + L[2, s]).astype(f32)
    assert np.array_equal(E[2], ((acc / f32(7)).astype(f32) * br.PI_F).astype(f32))
    d = rng.normal(size=(5, 7, 3))
    d = (d / np.linalg.norm(d, axis=2, keepdims=True)).astype(f32)
    C = br.fold_sh9(L, d)
    assert C.shape == (5, 9, 3)
    Y = br.sh9(d[4])
    acc = f32(0)
    for s in range(7):
        acc = f32(acc + f32(L[4, s, 1] * Y[s, 6]))
    assert C[4, 6, 1] == f32(f32(acc / f32(7)) * f32(f32(4.0) * br.PI_F))
    # against float64: a mean of 7 terms
    want = 4 * np.pi * np.einsum("nsc,nsk->nkc", L.astype(np.float64), br.sh9(d.reshape(-1, 3)).reshape(5, 7, 9).astype(np.float64)) / 7
    assert np.abs(C - want).max() <= 1e-4


def _edge_distance(uv, cx, cy):
    """distance of every centre to the nearest edge line segment of every triangle, float64: (T, Q)"""
    out = np.full((len(uv), len(cx)), np.inf)
    for i in range(3):
        a, b = uv[:, i, None, :], uv[:, (i + 1) % 3, None, :]
        ab = b - a
        p = np.stack([cx, cy], axis=-1)[None, :, :] - a
        den = np.maximum((ab * ab).sum(-1), 1e-300)
        t = np.clip((p * ab).sum(-1) / den, 0.0, 1.0)
        out = np.minimum(out, np.linalg.norm(p - t[..., None] * ab, axis=-1))
    return out


def atlases():
    """(name, lm_uv (T, 6), W, H): a hand-made atlas with both windings, and a random one"""
    hand = np.array([[0.05, 0.07, 0.61, 0.11, 0.33, 0.83], [0.9, 0.1, 0.55, 0.6, 0.95, 0.93], [0.1, 0.6, 0.3, 0.95, 0.02, 0.97]], dtype=f32)
    rng = np.random.default_rng(8)
    rand = rng.uniform(-0.1, 1.1, size=(12, 6)).astype(f32)
    return [("hand", hand, 37, 29), ("random", rand, 64, 48)]


@pytest.mark.parametrize("name,uv,W,H", atlases(), ids=[a[0] for a in atlases()])
def test_rasteriser_agrees_with_float64(name, uv, W, H):
    area, w0, w1, w2 = br.lightmap_weights(uv, W, H)
    got = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (area != 0)[:, None]
    u64 = uv.astype(np.float64).reshape(-1, 3, 2)
    q = np.arange(W * H)
    cx, cy = ((q % W) + 0.5) / W, ((q // W) + 0.5) / H

    def side(a, b):
        return (b[:, None, 0] - a[:, None, 0]) * (cy[None, :] - a[:, None, 1]) - (b[:, None, 1] - a[:, None, 1]) * (cx[None, :] - a[:, None, 0])

    s0, s1, s2 = side(u64[:, 0], u64[:, 1]), side(u64[:, 1], u64[:, 2]), side(u64[:, 2], u64[:, 0])
    inside = ((s0 >= 0) & (s1 >= 0) & (s2 >= 0)) | ((s0 <= 0) & (s1 <= 0) & (s2 <= 0))
    clear = _edge_distance(u64, cx, cy) > 1e-5
    assert np.array_equal(got[clear], inside[clear]), name
    band = np.count_nonzero(inside & ~clear)
    assert np.count_nonzero(inside) > 50 and band * 20 <= np.count_nonzero(inside), (name, band, np.count_nonzero(inside))


def test_lightmap_points_own_the_lowest_triangle_and_interpolate():
    # two triangles of one quad: the shared diagonal runs through texel centres, which the lower index owns
    uv = np.array([[0, 0, 1, 0, 1, 1], [0, 0, 1, 1, 0, 1]], dtype=f32)
    P = np.array([[0, 0, 0, 4, 0, 0, 4, 4, 0], [0, 0, 0, 4, 4, 0, 0, 4, 0]], dtype=f32)
    N = np.tile(np.array([0, 0, 2], dtype=f32), (2, 3)).reshape(2, 9)
    pts, tex = br.lightmap_points(P, N, uv, 4, 4)
    assert list(tex) == list(range(16)) and np.array_equal(pts["stream"], tex) and np.all(pts["reserved"] == 0)
    assert np.allclose(pts["position"][:, 0], (np.arange(16) % 4 + 0.5)) and np.allclose(pts["position"][:, 1], (np.arange(16) // 4 + 0.5))
    assert np.array_equal(pts["normal"], np.tile(np.array([0, 0, 1], dtype=f32), (16, 1)))
    area, w0, w1, w2 = br.lightmap_weights(uv, 4, 4)
    both = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)).all(axis=0)
    assert list(np.nonzero(both)[0]) == [0, 5, 10, 15]  # the diagonal's centres are covered by both: edges are inclusive
