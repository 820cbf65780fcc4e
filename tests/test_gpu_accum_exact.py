"""The accumulators' whole state and the adaptive controller, pinned exactly (include/rt_abi.h, "Resumable sample accumulators" and "The adaptive
rule, exactly"). S_p, E_p and n_p are compared bit for bit with the oracle's samples folded by the host model (adaptive_replay.fold), err with the
model's float32 err, and every adaptive call with adaptive_replay.replay on err tables that do not come from the call itself: the final count map,
the rounds, the samples added, the err of the last judge and the progress calls. Each replay scenario also shows that an injected fault of the
model changes its outcome, so the comparison can tell that fault from the rule."""
import ctypes as C
import os

import numpy as np
import pytest

import adaptive_replay as ar

pytestmark = pytest.mark.gpu

W, H = 64, 48
SEED = 7
N_ORACLE = 85  # samples per pixel the oracle provides for the 64x48 scenarios (the 0-defaults scenario reaches 80)
THREADS = min(16, int(os.environ.get("OMP_NUM_THREADS") or 16))
SEPARATING = ("lt", "border", "win5")


class _Case:
    """One scene at one image size: the oracle's samples of every pixel and the model's ladder and err tables built from them."""

    def __init__(self, dev, orc, w, h, n, seed=SEED):
        self.dev, self.w, self.h, self.seed = dev, w, h, seed
        self.x = orc.pixel_samples(w, h, n, np.arange(w * h), seed=seed, threads=THREADS).reshape(h, w, n, 3)
        self.S, self.E = ar.ladder(self.x)
        self.tab = ar.err_table(self.S, self.E)

    def at(self, n):
        """The model's S and E of a state whose pixel p holds n_p samples."""
        yy, xx = np.indices(n.shape)
        return self.S[n, yy, xx], self.E[n, yy, xx]

    def check_state(self, acc, what=""):
        r = acc.read()
        ar.assert_state(r, *self.at(r["samples"].astype(np.int64)), r["samples"], what=what)
        return r


def _adaptive(acc, thr, mn, mx, step, **kw):
    """One rt_accum_render_adaptive with its progress calls recorded: the outcome in the form replay() returns, and the stats."""
    calls = []
    st = acc.render_adaptive(thr, min_samples=mn, max_samples=mx, step=step, progress=lambda d, t: calls.append((int(d), int(t))), **kw)
    r = acc.read()
    return {"samples": r["samples"], "rounds": st["rounds"], "added": st["samples"], "error": r["error"], "progress": calls}, st


def _scenario(acc, tab, thr, mn, mx, step, n0, err0=None, need=(), what="", **kw):
    """Run an adaptive call and require the replay's outcome exactly. Then require some injected fault to change that outcome: one of SEPARATING
    or a stale err (the only one that can where no pixel is ever judged active: min == max, or every pixel past the cap), and each fault of
    `need` to change the count map."""
    want = ar.replay(n0, tab, thr, mn, mx, step, err0=err0)
    got, _ = _adaptive(acc, thr, mn, mx, step, **kw)
    ar.assert_replay(got, want, what=what)
    faults = {f: ar.replay(n0, tab, thr, mn, mx, step, fault=f, err0=err0) for f in SEPARATING + ("stale",)}
    assert any(ar.differs(faults[f], want) for f in faults), f"{what}: no injected fault changes this scenario"
    for f in need:
        assert not np.array_equal(faults[f]["samples"], want["samples"]), f"{what}: fault {f} gives the same map"
    return got, want


@pytest.fixture(scope="module")
def many(gpu, oracle, scenes):
    sc = scenes["room_manylights"]
    dev = gpu.DeviceScene(sc)
    orc = oracle.OracleScene(sc)
    case = _Case(dev, orc, W, H, N_ORACLE)
    case.orc = orc
    yield case
    dev.close()
    orc.close()


# ------------------------------------------------------------------------------------------------ C1: S, E, n against the oracle
def test_split_samples_at_odd_bases(many):
    acc = many.dev.accumulator(W, H, seed=SEED)
    total = 0
    for k in (1, 2, 3, 5):  # calls start at bases 0, 1, 3, 6
        acc.render(k)
        total += k
        many.check_state(acc, what=f"after {total}")
    acc.close()


def test_adaptive_after_render_then_uniform_on_a_mixed_map(many):
    acc = many.dev.accumulator(W, H, seed=SEED)
    acc.render(3)
    thr = ar.exact_threshold(many.tab, np.full((H, W), 3), 4, 14, 3)
    acc.render_adaptive(thr, min_samples=4, max_samples=14, step=3)  # round 0 adds one sample at base 3; later rounds start at 4, 7, ...
    n1 = many.check_state(acc, what="adaptive")["samples"]
    assert len(np.unique(n1)) >= 3 and (n1 % 2 == 1).any() and (n1 % 2 == 0).any()
    acc.render(5)  # odd and even bases in one call
    r = many.check_state(acc, what="uniform on top")
    assert np.array_equal(r["samples"], n1 + 5)
    acc.close()


def test_samples_cut_across_plans(many):
    w, h = 4, 3
    x = many.orc.pixel_samples(w, h, 1503, np.arange(w * h), seed=SEED, threads=THREADS).reshape(h, w, 1503, 3)
    acc = many.dev.accumulator(w, h, seed=SEED)
    acc.render(3)
    calls = []
    st = acc.render(1500, max_paths=1024, progress=lambda d, t: calls.append((int(d), int(t))))  # chunk 1024: plans at bases 3 and 1027
    assert st["samples"] == 1500 * w * h and st["passes"] == 24
    assert calls == [(i, 24) for i in range(1, 25)]
    ar.assert_state(acc.read(), *ar.fold(x), np.full((h, w), 1503), what="1503 in plans of 1024")
    acc.close()


# ------------------------------------------------------------------------------------------------ C2: err bit for bit
def _device_ladder(dev, w, h, levels, seed=SEED, **kw):
    """One accumulator, render(1) `levels` times: S, E at every level, and err read from a judge that adds nothing (min 2, max = the level,
    step 1), which must be the model's err of the S and E read back. Returns (S, E, err tables) indexed by level."""
    acc = dev.accumulator(w, h, seed=seed)
    S, E, tab = [np.zeros((h, w, 3), np.float32)], [np.zeros((h, w, 3), np.float32)], [np.full((h, w), np.inf, np.float32)]
    for L in range(1, levels + 1):
        acc.render(1, **kw)
        if L >= 2:
            st = acc.render_adaptive(0.0, min_samples=2, max_samples=L, step=1, **kw)
            assert st["rounds"] == 0 and st["samples"] == 0 and st["passes"] == 0
        r = acc.read()
        assert np.all(r["samples"] == L)
        model = ar.err(r["sum"], r["even_sum"], L)
        if L >= 2:
            ar.assert_floats_equal(r["error"], model, f"err at level {L}")
        S.append(r["sum"])
        E.append(r["even_sum"])
        tab.append(model)
    acc.close()
    return np.stack(S), np.stack(E), np.stack(tab)


def test_err_kernel_is_the_model_at_every_level(many):
    S, E, tab = _device_ladder(many.dev, W, H, 24)
    ar.assert_floats_equal(S, many.S[:25], "ladder S")
    ar.assert_floats_equal(E, many.E[:25], "ladder E")
    ar.assert_floats_equal(tab, many.tab[:25], "ladder err")


# ------------------------------------------------------------------------------------------------ C3: adaptive replay, parity
def test_replay_exact_err_threshold(many):
    z = np.zeros((H, W), int)
    thr = ar.exact_threshold(many.tab, z, 4, 24, 4)
    assert np.float32(thr) in many.tab[4]
    acc = many.dev.accumulator(W, H, seed=SEED)
    got, _ = _scenario(acc, many.tab, thr, 4, 24, 4, z, need=("lt",), what="exact err threshold")
    assert got["rounds"] >= 3 and 4 < got["samples"].mean() < 24
    many.check_state(acc, what="exact err threshold")
    # a second call with a lower threshold resumes from the first call's map and err
    thr2 = float(np.float32(thr) / np.float32(2))
    got2, _ = _scenario(acc, many.tab, thr2, 4, 32, 4, got["samples"], err0=got["error"], what="second call")
    assert (got2["samples"] > got["samples"]).any()
    many.check_state(acc, what="second call")
    acc.close()


@pytest.mark.parametrize("mn,mx,step,q", [(4, 13, 4, 0.5), (8, 8, 4, 0.5), (0, 80, 0, 0.5)], ids=["cap-off-step", "min-eq-max", "defaults"])
def test_replay_levels(many, mn, mx, step, q):
    z = np.zeros((H, W), int)
    thr = ar.exact_threshold(many.tab, z, mn, mx, step, q=q, need=() if mn == mx else ("lt",))
    acc = many.dev.accumulator(W, H, seed=SEED)
    got, _ = _scenario(acc, many.tab, thr, mn, mx, step, z, what=f"{mn}/{mx}/{step}")
    levels = set(np.unique(got["samples"]).tolist())
    if (mn, mx, step) == (4, 13, 4):
        assert levels <= {4, 8, 12, 13} and 13 in levels
    elif mn == mx:
        assert levels == {8} and got["rounds"] == 1 and got["progress"] == [(1, 1)]
    else:
        assert levels <= {16, 48, 80} and len(levels) >= 2
    many.check_state(acc, what=f"{mn}/{mx}/{step}")
    acc.close()


def test_replay_resumed_below_min_and_past_the_cap(many):
    acc = many.dev.accumulator(W, H, seed=SEED)
    acc.render(3)
    n0 = np.full((H, W), 3)
    thr = ar.exact_threshold(many.tab, n0, 6, 18, 4)
    _scenario(acc, many.tab, thr, 6, 18, 4, n0, what="from render(3)")  # round 0 adds 3 samples at base 3
    many.check_state(acc, what="from render(3)")
    acc.close()
    acc = many.dev.accumulator(W, H, seed=SEED)
    acc.render(20)
    assert np.all(np.isinf(acc.read()["error"]))
    got, want = _scenario(acc, many.tab, 0.01, 4, 16, 4, np.full((H, W), 20), what="past the cap")
    assert got["rounds"] == 0 and got["added"] == 0 and got["progress"] == []
    ar.assert_floats_equal(got["error"], many.tab[20], "refreshed err")  # what the stale-err fault would not have
    acc.close()


def test_replay_threshold_zero(gpu, oracle, scenes):
    """Threshold 0 on a scene with windows of err exactly 0 (faces of constant radiance): only they stop below the cap."""
    sc = scenes["boxes"]
    dev = gpu.DeviceScene(sc)
    orc = oracle.OracleScene(sc)
    case = _Case(dev, orc, W, H, 12)
    z = np.zeros((H, W), int)
    acc = dev.accumulator(W, H, seed=SEED)
    got, _ = _scenario(acc, case.tab, 0.0, 4, 12, 4, z, need=("lt",), what="threshold 0")
    assert (got["samples"] < 12).any() and (got["samples"] == 12).any()
    case.check_state(acc, what="threshold 0")
    dev.close()
    orc.close()


@pytest.mark.parametrize("shape", [(1, 37), (53, 1), (1, 1), (2, 2), (257, 3)])  # (width, height)
def test_replay_shapes(many, shape):
    w, h = shape
    case = _Case(many.dev, many.orc, w, h, 17)
    z = np.zeros((h, w), int)
    thr = ar.exact_threshold(case.tab, z, 2, 14, 3, level=2)
    acc = many.dev.accumulator(w, h, seed=SEED)
    _scenario(acc, case.tab, thr, 2, 14, 3, z, need=("lt",), what=f"{w}x{h}")
    case.check_state(acc, what=f"{w}x{h}")
    acc.render(3)
    case.check_state(acc, what=f"{w}x{h} + 3")
    acc.close()


# ------------------------------------------------------------------------------------------------ C4: production traversals
@pytest.mark.parametrize("mode", ["global_best", "wide"])
def test_replay_production(gpu, scenes, mode):
    sc = scenes["room_manylights"]
    dev = gpu.DeviceScene(sc, **({"device_bvh": True, "wide": True} if mode == "wide" else {}))
    S, E, tab = _device_ladder(dev, W, H, 24, global_best=True)
    z = np.zeros((H, W), int)
    thr = ar.exact_threshold(tab, z, 4, 24, 4)
    acc = dev.accumulator(W, H, seed=SEED)
    got, _ = _scenario(acc, tab, thr, 4, 24, 4, z, need=("lt",), what=f"{mode} exact err threshold", global_best=True)
    yy, xx = np.indices((H, W))
    n = got["samples"].astype(np.int64)
    ar.assert_state(acc.read(), S[n, yy, xx], E[n, yy, xx], n, what=mode)
    acc.close()
    acc = dev.accumulator(W, H, seed=SEED)
    acc.render(3, global_best=True)
    n0 = np.full((H, W), 3)
    thr = ar.exact_threshold(tab, n0, 4, 13, 4)
    _scenario(acc, tab, thr, 4, 13, 4, n0, what=f"{mode} from render(3), cap off the step", global_best=True)
    dev.close()


# ------------------------------------------------------------------------------------------------ C5: more than 2^20 pixels
def test_more_than_2_20_pixels(gpu, oracle, scenes):
    w, h = 1032, 1024
    n_pix = w * h
    assert n_pix > (1 << 20) and n_pix % 256 == 0 and n_pix > 4096 * 256
    sc = scenes["room_manylights"]
    dev = gpu.DeviceScene(sc)
    S, E, tab = _device_ladder(dev, w, h, 4)
    z = np.zeros((h, w), int)
    thr = ar.exact_threshold(tab, z, 2, 4, 1, q=0.8)
    acc = dev.accumulator(w, h, seed=SEED)
    got, _ = _scenario(acc, tab, thr, 2, 4, 1, z, what="1032x1024")
    assert set(np.unique(got["samples"]).tolist()) == {2, 3, 4}
    r = acc.read()
    acc.close()
    # the oracle on ~2000 pixels: the last 1000, those around 2^20, and a random spread
    pick = np.unique(np.concatenate([np.arange(n_pix - 1000, n_pix), np.arange((1 << 20) - 300, (1 << 20) + 300),
                                     np.random.default_rng(5).integers(0, n_pix, 400)]))
    orc = oracle.OracleScene(sc)
    x = orc.pixel_samples(w, h, 4, pick, seed=SEED, threads=THREADS)
    orc.close()
    OS, OE = ar.ladder(x)
    n = r["samples"].reshape(-1)[pick].astype(np.int64)
    ar.assert_floats_equal(r["sum"].reshape(-1, 3)[pick], OS[n, np.arange(len(pick))], "S at sampled pixels")
    ar.assert_floats_equal(r["even_sum"].reshape(-1, 3)[pick], OE[n, np.arange(len(pick))], "E at sampled pixels")
    for L in range(1, 5):  # the ladder the tables came from
        ar.assert_floats_equal(S[L].reshape(-1, 3)[pick], OS[L], f"ladder S at level {L}")
        ar.assert_floats_equal(E[L].reshape(-1, 3)[pick], OE[L], f"ladder E at level {L}")
    dev.close()


# ------------------------------------------------------------------------------------------------ C6: overflowing light
def test_overflowing_light_sends_nan_windows_to_the_cap(gpu, oracle, sg):
    from conftest import golden_scene_specs, make_scene

    spec = dict(golden_scene_specs()["room_plain"], light_strength=3e38)
    sc = make_scene(sg, spec)
    dev = gpu.DeviceScene(sc)
    orc = oracle.OracleScene(sc)
    case = _Case(dev, orc, W, H, 10)
    # the case is real: some S overflows to +inf and its err is NaN, while other pixels keep a finite err
    inf_px = np.isinf(case.S[4]).any(-1)
    assert inf_px.any() and np.isnan(case.tab[4][inf_px]).all() and np.isfinite(case.tab[4]).sum() > W * H // 4
    z = np.zeros((H, W), int)
    # NaN windows cover most of the image: a high threshold leaves some clean windows below the cap, and a 5x5 window would not
    thr = ar.exact_threshold(case.tab, z, 2, 10, 2, q=0.9, need=("win5",))
    acc = dev.accumulator(W, H, seed=SEED)
    got, _ = _scenario(acc, case.tab, thr, 2, 10, 2, z, need=("win5",), what="overflowing light")
    nan_win = ar.unconverged_windows(np.where(np.isnan(got["error"]), np.float32(np.inf), np.float32(0)), np.float32(0), None)
    assert nan_win.any() and np.all(got["samples"][nan_win] == 10) and (got["samples"] < 10).any()
    case.check_state(acc, what="overflowing light")
    dev.close()
    orc.close()


# ------------------------------------------------------------------------------------------------ C7: counters and progress
def test_counters_of_split_calls_equal_the_oracle(gpu, many):
    acc = many.dev.accumulator(W, H, seed=SEED)
    keys = ("samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests",
            "light_tri_tests", "light_hits", "texel_fetches")
    tot = dict.fromkeys(keys, 0)
    for k in (3, 5, 8):
        st = acc.render(k, counters=True)
        assert st["samples"] == k * W * H
        for key in keys:
            tot[key] += st[key]
    _, ost = many.orc.run_raytracer(W, H, 16, rng_mode=gpu.RT_RNG_DEVICE, seed=SEED, threads=THREADS)
    for key in keys:
        assert tot[key] == ost[key], f"counter {key}: accumulator {tot[key]} oracle {ost[key]}"
    acc.close()


def test_progress_of_a_multi_pass_render(many):
    acc = many.dev.accumulator(W, H, seed=SEED)
    calls = []
    st = acc.render(4, max_paths=1024, progress=lambda d, t: calls.append((int(d), int(t))))
    N = st["passes"]
    assert N == 12 and calls == [(i, N) for i in range(1, N + 1)]
    acc.close()


# ------------------------------------------------------------------------------------------------ C8: device destinations
def test_resolve_into_device_buffers(gpu, many):
    import torch

    lib, abi = gpu.lib(), gpu._ctypes_abi
    acc = many.dev.accumulator(W, H, seed=SEED)
    acc.render(3)
    acc.render_adaptive(ar.exact_threshold(many.tab, np.full((H, W), 3), 4, 12, 4), min_samples=4, max_samples=12, step=4)
    fb = torch.full((H * W * 3,), -1.0, dtype=torch.float32, device="cuda")
    rgb8 = torch.full((H * W * 3,), 7, dtype=torch.uint8, device="cuda")
    assert lib.rt_accum_resolve(acc._h, abi.RT_FLAG_DEVICE_FB, C.c_void_p(fb.data_ptr())) == 0
    assert lib.rt_accum_resolve_rgb8(acc._h, abi.RT_FLAG_DEVICE_FB, C.c_void_p(rgb8.data_ptr())) == 0
    torch.cuda.synchronize()
    img = acc.image()
    assert np.array_equal(fb.cpu().numpy().reshape(H, W, 3).view(np.uint32), img.view(np.uint32))
    assert np.array_equal(rgb8.cpu().numpy().reshape(H, W, 3), acc.image(rgb8=True))
    n = acc.read()["samples"].astype(np.int64)
    S, _ = many.at(n)
    assert np.array_equal(img.view(np.uint32), (S / n.astype(np.float32)[..., None]).view(np.uint32))
    acc.close()
