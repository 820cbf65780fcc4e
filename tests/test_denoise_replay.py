"""The host model of rt_accum_denoise (tests/denoise_replay.py) held to the properties the rule (include/rt_abi.h) is built for, on
synthetic accumulator states, and every injected fault of the model shown to change the output of at least one of these cases: the GPU
tests compare the device with this model bit for bit, so what holds here holds for the kernels."""
import numpy as np
import pytest

import denoise_replay as dr

H, W = 24, 32
F = np.float32


def _state(n, C, alb, nrm, z, hit_frac=None, noise=0.0, seed=3):
    """An accumulator state with n_p samples per pixel whose means are C (image), alb, nrm, and depth z on the hit samples; E is the sum of the
    even-index half, perturbed by `noise` (relative) so that the half-buffer difference is not zero."""
    rng = np.random.default_rng(seed)
    n = np.broadcast_to(np.asarray(n), (H, W)).astype(np.uint32)
    fn = n.astype(F)
    hits = n.copy() if hit_frac is None else np.minimum(n, np.round(fn * hit_frac).astype(np.uint32))
    S = (np.asarray(C, F) * fn[..., None]).astype(F)
    half = ((n + 1) // 2).astype(F)
    E = (np.asarray(C, F) * half[..., None] * (1 + noise * rng.standard_normal((H, W, 3))).astype(F)).astype(F)
    AS = (np.asarray(alb, F) * fn[..., None]).astype(F)
    NS = (np.asarray(nrm, F) * fn[..., None]).astype(F)
    ZS = (np.asarray(z, F) * hits.astype(F)).astype(F)
    return dict(S=S, E=E, n=n, AS=AS, NS=NS, ZS=ZS, hits=hits)


def _run(st, **kw):
    return dr.denoise(st["S"], st["E"], st["n"], st["AS"], st["NS"], st["ZS"], st["hits"], **kw)


def _full(v):
    return np.broadcast_to(np.asarray(v, F), (H, W, 3)).copy()


def _ulps(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()


@pytest.fixture(scope="module")
def cases():
    """name -> (state, options, function of the output that the case is about). Used by the property tests and by the fault matrix."""
    rng = np.random.default_rng(11)
    out = {}
    # a constant image under arbitrary guides
    nrm = rng.standard_normal((H, W, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    out["constant"] = (_state(rng.integers(2, 9, (H, W)), _full((0.5, 0.25, 0.125)), _full(0.0), nrm, rng.uniform(1, 20, (H, W)), noise=0.3), dict(demodulate=False))
    # two halves with opposite normals and different colours
    left = np.arange(W)[None, :, None] < W // 2
    # (the 3x3 window of the noise scale s_p is not edge-aware by the rule, so the case keeps d_q the same exact number in every pixel: colours
    # on a grid of 1/64, A = C + 1/8 per channel, no demodulation -> d = 3/8 and s = 3/8 whatever the window holds)
    C = np.round(64 * (np.where(left, _full((0.9, 0.2, 0.1)), _full((0.1, 0.3, 0.8))) + 0.1 * rng.standard_normal((H, W, 3)))) / 64
    halves = _state(4, np.abs(C).astype(F), _full(0.5), np.where(left, _full((0, 0, 1)), _full((0, 0, -1))), 5.0)
    halves["E"] = ((np.abs(C).astype(F) + F(0.125)) * F(2)).astype(F)
    out["halves"] = (halves, dict(demodulate=False))
    # a depth step with equal normals
    z = np.where(np.arange(W)[None, :] < W // 2, F(2), F(8)) * np.ones((H, W), F)
    Cz = np.where(left, _full(1.0), _full(0.0))
    out["depth_step"] = (_state(4, Cz, _full(0.5), _full((0, 0, 1)), z, noise=0.0), dict(iterations=1, demodulate=False))
    # invalid pixels scattered through a noisy image, and pixels with one sample
    n = rng.integers(2, 9, (H, W))
    n[rng.random((H, W)) < 0.15] = 0
    n[rng.random((H, W)) < 0.10] = 1
    n[0, 0], n[H - 1, W - 1], n[0, W - 1] = 0, 1, 3
    Cn = (0.5 + 0.3 * rng.standard_normal((H, W, 3))).astype(F)
    out["holes"] = (_state(n, np.abs(Cn), _full(0.6), _full((0, 1, 0)), rng.uniform(4, 5, (H, W)), hit_frac=0.75, noise=0.3), {})
    return out


def test_constant_image_stays_constant(cases):
    st, kw = cases["constant"]
    got = _run(st, **kw)
    want = (st["S"] / st["n"].astype(F)[..., None]).astype(F)
    assert _ulps(got, want) <= 2  # a weighted mean of equal values: the division of two rounded sums


def test_opposite_normals_do_not_mix(cases):
    st, kw = cases["halves"]
    got = _run(st, **kw)
    for side in (slice(0, W // 2), slice(W // 2, W)):
        alone = {k: (v[:, side] if v.ndim >= 2 else v) for k, v in st.items()}
        want = dr.denoise(alone["S"], alone["E"], alone["n"], alone["AS"], alone["NS"], alone["ZS"], alone["hits"], **kw)
        assert np.array_equal(got[:, side].view(np.uint32), want.view(np.uint32))  # bit-equal to filtering the side alone
    assert np.abs(got - st["S"] / F(4)).max() > 1e-3  # and it did filter


def test_depth_step_is_attenuated_as_wz_says(cases):
    """One iteration, no colour noise (s = 0 would make wc a step; here the image is constant on each side, so only wz couples the sides): a
    pixel next to the step mixes in the other side with exactly the weights k * wz."""
    st, kw = cases["depth_step"]
    st = dict(st)
    st["E"] = (st["S"] / F(4) * F(2) * F(1.5)).astype(F)  # a large half-buffer difference: wc ~ 1 across the step
    got = _run(st, sigma_color=1e6, **kw)
    x, y = W // 2 - 1, H // 2  # last column of the near side: taps dx = +1, +2 lie on the far side
    k = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    wz = lambda dist: 1.0 / (1.0 + ((2.0 - 8.0) / (0.5 * dist * 8.0)) ** 2)
    num = den = 0.0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            far = dx >= 1
            w = k[dy + 2] * k[dx + 2] * (wz(max(abs(dx), abs(dy))) if far else 1.0)
            num += w * (0.0 if far else 1.0)
            den += w
    assert abs(float(got[y, x, 0]) - num / den) < 1e-5
    assert 11 / 16 + 1e-3 < float(got[y, x, 0]) < 1.0 - 1e-3  # attenuated, not cut: between full mixing (11/16) and none
    same = dr.denoise(st["S"], st["E"], st["n"], st["AS"], st["NS"], np.full((H, W), 8.0, F) * st["hits"], st["hits"], sigma_color=1e6, **kw)
    assert float(same[y, x, 0]) < float(got[y, x, 0])  # without the step the far side mixes in fully


def test_invalid_pixels_are_skipped(cases):
    st, kw = cases["holes"]
    got = _run(st, **kw)
    hole = st["n"] == 0
    assert hole.sum() > 20 and not got[hole].any()
    assert np.isfinite(got).all()
    # what an invalid pixel holds never matters
    st2 = {k: v.copy() for k, v in st.items()}
    for k in ("S", "E", "AS", "NS"):
        st2[k][hole] = 1e30
    st2["ZS"][hole] = 1e30
    st2["hits"][hole] = 0
    assert np.array_equal(_run(st2, **kw).view(np.uint32), got.view(np.uint32))


def test_single_sample_pixels_are_filtered_by_geometry_alone(cases):
    st, kw = cases["holes"]
    P = dr.prepare(st["S"], st["E"], st["n"], st["AS"], st["NS"], st["ZS"], st["hits"])
    one = st["n"] == 1
    assert one.sum() > 10 and np.isinf(P["s"][one]).all()  # d = +inf enters the window mean
    got = _run(st, **kw)
    other = _run(st, sigma_color=0.25, **kw)  # wc = 1 for them whatever sigma_color: only their neighbours' own wc changes L
    first = dr.iterate(P, P["L0"], 0, 4.0, 0.5, 3), dr.iterate(P, P["L0"], 0, 0.25, 0.5, 3)
    assert np.array_equal(first[0][one].view(np.uint32), first[1][one].view(np.uint32))
    assert not np.array_equal(got.view(np.uint32), other.view(np.uint32))


def test_every_fault_changes_some_case(cases):
    for fault in dr.FAULTS:
        changed = [name for name, (st, kw) in cases.items() if not np.array_equal(_run(st, fault=fault, **kw).view(np.uint32), _run(st, **kw).view(np.uint32))]
        assert changed, f"fault {fault} changes no case"
