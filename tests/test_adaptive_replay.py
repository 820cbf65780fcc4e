"""CPU tests of what the exact accumulator tests (test_gpu_accum_exact.py) are built on: the oracle's per-sample radiance (OracleScene.pixel_samples)
is the stream run_raytracer folds, and the host model of the contract (adaptive_replay.py) states the adaptive rule of include/rt_abi.h. Every
variant of the model a subtly wrong kernel would follow (adaptive_replay.FAULTS) is injected and must make the comparison helpers raise."""
import os

import numpy as np
import pytest

import adaptive_replay as ar

FIXTURES = ["room_plain", "room_textured", "open_nolight", "boxes", "room_manylights"]
THREADS = min(16, int(os.environ.get("OMP_NUM_THREADS") or 16))
INF = np.float32(np.inf)


@pytest.mark.parametrize("name", FIXTURES)
def test_pixel_samples_fold_to_the_oracle_image(oracle, scenes, name):
    W, H, N, seed = 40, 24, 5, 17
    orc = oracle.OracleScene(scenes[name])
    fb, _ = orc.run_raytracer(W, H, N, seed=seed, threads=THREADS)
    x = orc.pixel_samples(W, H, N, np.arange(W * H), seed=seed, threads=THREADS)
    assert x.shape == (W * H, N, 3) and x.dtype == np.float32 and not np.isnan(x).any()
    S, _ = ar.fold(x)
    assert np.array_equal((S / np.float32(N)).reshape(H, W, 3).view(np.uint32), fb.view(np.uint32))
    # a list out of order, with a repeat: each row is that pixel's stream, whatever its position
    idx = np.random.default_rng(3).permutation(W * H)[:97]
    idx = np.concatenate([idx, idx[:5]])
    y = orc.pixel_samples(W, H, N, idx, seed=seed, threads=3)
    assert np.array_equal(y.view(np.uint32), x[idx].view(np.uint32))
    # another seed is another stream
    assert not np.array_equal(orc.pixel_samples(W, H, N, idx[:20], seed=seed + 1, threads=THREADS), y[:20])
    with pytest.raises(RuntimeError, match="outside the image"):
        orc.pixel_samples(W, H, N, [W * H], seed=seed)
    orc.close()


def test_fold_ladder_and_err_by_hand():
    # 0.1 + 0.2 + 0.3 in binary32 order differs from the pairwise / double sums: the fold is sequential
    v = np.array([0.1, 0.2, 0.3, 1e8, -1e8, 0.7], dtype=np.float32)
    x = np.stack([v, v * 2, v * 3], axis=-1)[None]
    S, E = ar.fold(x)
    want_s = np.float32(0)
    for a in v:
        want_s = np.float32(want_s + a)
    assert S[0, 0] == want_s and E[0, 0] == np.float32(np.float32(np.float32(0.1) + np.float32(0.3)) + np.float32(-1e8))
    Sl, El = ar.ladder(x)
    for L in range(len(v) + 1):
        s, e = ar.fold(x[:, :L])
        assert np.array_equal(Sl[L].view(np.uint32), s.view(np.uint32)) and np.array_equal(El[L].view(np.uint32), e.view(np.uint32))
        s2, e2 = ar.fold(x, counts=np.array([L]))
        assert np.array_equal(s2.view(np.uint32), s.view(np.uint32)) and np.array_equal(e2.view(np.uint32), e.view(np.uint32))
    # err: +inf below 2 samples; a constant stream has err 0; the formula, operation for operation, on one pixel
    assert np.isinf(ar.err(Sl[1], El[1], 1)).all() and np.isinf(ar.err(Sl[0], El[0], 0)).all()
    c = np.full((1, 7, 3), 0.25, dtype=np.float32)
    s, e = ar.fold(c)
    assert ar.err(s, e, 7)[0] == 0.0
    s, e = np.array([3.0, 1.5, 0.75], np.float32), np.array([2.0, 0.5, 1.0], np.float32)
    I, A = s / np.float32(5), e / np.float32(3)
    d = np.abs(I - A)
    want = np.float32(np.float32(np.float32(d[0] + d[1]) + d[2]) / np.float32(np.float32(1e-4) + np.sqrt(np.float32(np.float32(I[0] + I[1]) + I[2]))))
    assert ar.err(s, e, 5) == want and np.float32(1e-4).view(np.uint32) == 0x38D1B717  # the bits of the device's 1e-4f


def _const_table(e, levels=300):
    """err tables that do not depend on the level: err_q = e[q] whatever n_q (levels below 2 stay +inf)."""
    e = np.asarray(e, dtype=np.float32)
    return [np.full(e.shape, INF)] * 2 + [e] * (levels - 2)


@pytest.mark.parametrize("shape", [(5, 7), (1, 9), (8, 1), (1, 1), (2, 2)])
def test_one_unconverged_pixel_activates_its_clipped_window(shape):
    H, W = shape
    for q in {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, 0), (0, W // 2), (H // 2, W // 2)}:
        e = np.zeros(shape, dtype=np.float32)
        e[q] = 1.0
        rep = ar.replay(np.zeros(shape, int), _const_table(e), 0.5, 2, 3, 1)
        win = np.zeros(shape, dtype=bool)
        win[max(q[0] - 1, 0):q[0] + 2, max(q[1] - 1, 0):q[1] + 2] = True
        assert np.array_equal(rep["samples"], np.where(win, 3, 2)), (shape, q)
        assert rep["rounds"] == 2 and rep["added"] == 2 * H * W + int(win.sum()) and rep["progress"] == [(1, 2), (2, 2)]
        assert ar.differs(rep, ar.replay(np.zeros(shape, int), _const_table(e), 0.5, 2, 3, 1, fault="win5")) == (H > 2 or W > 2)


def test_nan_is_unconverged_and_equal_is_converged():
    e = np.full((3, 4), 0.25, dtype=np.float32)
    rep = ar.replay(np.zeros((3, 4), int), _const_table(e), 0.25, 2, 6, 2)
    assert np.all(rep["samples"] == 2) and rep["rounds"] == 1 and rep["progress"] == [(1, 3)]
    assert np.all(ar.replay(np.zeros((3, 4), int), _const_table(e), 0.25, 2, 6, 2, fault="lt")["samples"] == 6)
    e[0, 3] = np.nan
    rep = ar.replay(np.zeros((3, 4), int), _const_table(e), 0.25, 2, 6, 2)
    assert np.array_equal(rep["samples"], [[2, 2, 6, 6], [2, 2, 6, 6], [2, 2, 2, 2]]) and rep["rounds"] == 3
    assert np.isnan(rep["error"][0, 3]) and (rep["error"][~np.isnan(rep["error"])] == 0.25).all()


def test_levels_caps_and_defaults():
    e = np.full((2, 3), 9.0, dtype=np.float32)  # never converged: every pixel walks the whole ladder
    tab = _const_table(e)
    z = np.zeros((2, 3), int)
    rep = ar.replay(z, tab, 1.0, 4, 13, 4)  # the cap not reached by whole steps: 4, 8, 12, 13
    assert np.all(rep["samples"] == 13) and rep["rounds"] == 4 and rep["added"] == 6 * 13
    assert rep["progress"] == [(1, 4), (2, 4), (3, 4), (4, 4)]
    rep = ar.replay(z, tab, 1.0, 8, 8, 4)  # min == max: round 0 only
    assert np.all(rep["samples"] == 8) and rep["rounds"] == 1 and rep["progress"] == [(1, 1)]
    rep = ar.replay(z, tab, 1.0, 0, 80, 0)  # 0 = 16 for min, 32 for step: 16, 48, 80
    assert np.all(rep["samples"] == 80) and rep["rounds"] == 3 and rep["progress"] == [(1, 3), (2, 3), (3, 3)]
    # counts above the cap are never active; round 0 tops up unequal counts to min and leaves the rest
    n0 = np.array([[0, 3, 5], [20, 12, 7]])
    rep = ar.replay(n0, tab, 1.0, 6, 12, 4)
    assert np.array_equal(rep["samples"], [[12, 12, 12], [20, 12, 12]])
    assert rep["added"] == int((rep["samples"] - n0).sum()) and rep["rounds"] == 3
    rep = ar.replay(np.full((2, 3), 20), tab, 1.0, 4, 16, 4)  # all past the cap: nothing added, err judged once on the state
    assert rep["rounds"] == 0 and rep["added"] == 0 and rep["progress"] == [] and np.array_equal(rep["error"], e)


def test_progress_total_grows_when_neighbours_reactivate():
    # 1x5: pixel 0 never converges, every pixel at the cap stops converging; activity spreads one pixel per three rounds
    W, mx = 5, 8
    tab = [np.full((1, W), INF)] * 2 + [np.zeros((1, W), np.float32)] * 6 + [np.full((1, W), 9.0, np.float32)] * 4
    tab[2] = tab[4] = tab[6] = np.where(np.arange(W) == 0, np.float32(9.0), np.float32(0.0))[None]
    rep = ar.replay(np.zeros((1, W), int), tab, 1.0, 2, mx, 2)
    assert np.all(rep["samples"] == mx)
    bound = 1 + 3
    assert rep["rounds"] > bound and rep["progress"] == [(r, max(r, bound)) for r in range(1, rep["rounds"] + 1)]


@pytest.fixture(scope="module")
def fixture_state(oracle, scenes):
    """room_manylights at 32x24: the oracle's samples, the ladder of S / E and its err tables."""
    W, H, N, seed = 32, 24, 20, 7
    orc = oracle.OracleScene(scenes["room_manylights"])
    x = orc.pixel_samples(W, H, N, np.arange(W * H), seed=seed, threads=THREADS).reshape(H, W, N, 3)
    orc.close()
    S, E = ar.ladder(x)
    return x, S, E, ar.err_table(S, E)


def test_injected_faults_raise(fixture_state):
    x, S, E, tab = fixture_state
    H, W = tab.shape[1:]
    z = np.zeros((H, W), int)
    # the exact model passes its own comparisons
    mn, mx, step = 4, 16, 4
    thr = ar.exact_threshold(tab, z, mn, mx, step)
    rep = ar.replay(z, tab, thr, mn, mx, step)
    ar.assert_replay(rep, rep)
    ar.assert_state({"samples": np.full((H, W), 11, np.uint32), "sum": S[11], "even_sum": E[11]}, *ar.fold(x[:, :, :11]), np.full((H, W), 11))
    assert 4 < rep["samples"].mean() < 16 and rep["rounds"] >= 2
    # judge faults: < for <=, a 5x5 window, the border unconverged, a stale err
    for f in ar.JUDGE_FAULTS:
        with pytest.raises(AssertionError, match="count map|err"):
            ar.assert_replay(ar.replay(z, tab, thr, mn, mx, step, fault=f), rep, what=f)
    # E by the parity within each call (1, 2, 3, 5 samples: calls that start at odd bases)
    bad_S, bad_E = ar.fold(x[:, :, :11], fault="local_parity", chunks=(1, 2, 3, 5))
    assert np.array_equal(bad_S, S[11])
    with pytest.raises(AssertionError, match=" E: "):
        ar.assert_state({"samples": np.full((H, W), 11, np.uint32), "sum": bad_S, "even_sum": bad_E}, S[11], E[11], np.full((H, W), 11))
    # h = n // 2: another err at every odd level, so another err read back and another replay
    bad_tab = ar.err_table(S, E, fault="h_floor")
    with pytest.raises(AssertionError, match="err"):
        ar.assert_floats_equal(bad_tab[5], tab[5], "err")
    assert np.array_equal(bad_tab[6].view(np.uint32), tab[6].view(np.uint32))
    with pytest.raises(AssertionError, match="count map|err"):
        ar.assert_replay(ar.replay(z, bad_tab, thr, mn, 13, step), ar.replay(z, tab, thr, mn, 13, step))
    # a wrong n, a last-bit S, a wrong round count and a missing progress call
    st = {"samples": np.full((H, W), 11, np.uint32), "sum": S[11].copy(), "even_sum": E[11]}
    st["sum"][3, 4, 1] = np.nextafter(st["sum"][3, 4, 1], np.float32(np.inf))
    with pytest.raises(AssertionError, match=r"S: 1 values differ; first at \(3, 4, 1\)"):
        ar.assert_state(st, S[11], E[11], np.full((H, W), 11))
    st["samples"] = st["samples"].copy()
    st["samples"][0, 0] = 12
    with pytest.raises(AssertionError, match="n: 1 pixels differ"):
        ar.assert_state(st, S[11], E[11], np.full((H, W), 11))
    with pytest.raises(AssertionError, match="rounds"):
        ar.assert_replay(dict(rep, rounds=rep["rounds"] + 1), rep)
    with pytest.raises(AssertionError, match="progress"):
        ar.assert_replay(dict(rep, progress=rep["progress"][:-1]), rep)


def test_exact_threshold_separates_lt(fixture_state):
    _, _, _, tab = fixture_state
    z = np.zeros(tab.shape[1:], int)
    thr = ar.exact_threshold(tab, z, 4, 12, 4)
    assert np.float32(thr) in tab[4]
    assert ar.differs(ar.replay(z, tab, thr, 4, 12, 4), ar.replay(z, tab, thr, 4, 12, 4, fault="lt"))
