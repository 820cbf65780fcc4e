"""A host model of the accumulator contract (include/rt_abi.h, "Resumable sample accumulators" and "The adaptive rule, exactly"), for exact
comparisons with the device. A plain module next to the tests (imported like hit_contract.py).
  fold / ladder  S_p and E_p of a pixel's samples: binary32 additions in sample order from +0.0, E over the even ABSOLUTE sample indices;
  err            the half-buffer error, one numpy float32 operation for each operation the header states;
  replay         the adaptive rule round by round on per-level err tables: the final count map, the rounds, the samples added, the err the
                 last judge saw and the progress calls the device must make.
`fault=` selects a variant of the model that a subtly wrong kernel would follow (FAULTS). The CPU tests require every variant to make the
comparison helpers raise on a fixture, so a GPU test that compares the device with the exact model and passes has ruled each of them out."""
import numpy as np

JUDGE_FAULTS = ("lt", "win5", "border", "stale")  # err < thr for err <= thr; a 5x5 window; the border counted unconverged; err one round old
STATE_FAULTS = ("local_parity", "h_floor")  # E by the parity of the index within a call; h = n // 2
FAULTS = JUDGE_FAULTS + STATE_FAULTS


def fold(samples, counts=None, fault=None, chunks=None):
    """samples (..., N, 3) in sample order -> (S, E), each (..., 3) float32. `counts` (...): fold only the first n_p samples of each pixel.
    fault="local_parity" with `chunks` (the sample counts of successive calls): E takes the even indices within each call instead."""
    x = np.asarray(samples, dtype=np.float32)
    N = x.shape[-2]
    n = np.full(x.shape[:-2], N, dtype=np.int64) if counts is None else np.asarray(counts).astype(np.int64)
    idx = _local_index(N, chunks) if fault == "local_parity" else np.arange(N)
    S = np.zeros(x.shape[:-2] + (3,), dtype=np.float32)
    E = np.zeros_like(S)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(N):  # one binary32 addition per sample, in order (np.sum would add pairwise)
            take = (s < n)[..., None]
            v = x[..., s, :]
            S = np.where(take, S + v, S)
            if idx[s] % 2 == 0:
                E = np.where(take, E + v, E)
    return S, E


def ladder(samples):
    """(S, E) of every prefix of the samples: arrays (N + 1, ..., 3), level L holding the fold of samples 0 .. L - 1."""
    x = np.asarray(samples, dtype=np.float32)
    S = [np.zeros(x.shape[:-2] + (3,), dtype=np.float32)]
    E = [S[0]]
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(x.shape[-2]):
            v = x[..., s, :]
            S.append(S[-1] + v)
            E.append(E[-1] + v if s % 2 == 0 else E[-1])
    return np.stack(S), np.stack(E)


def err(S, E, n, fault=None):
    """err_p of the header in float32: I = S/n, A = E/h (h = (n + 1) // 2), ((|dI.r| + |dI.g|) + |dI.b|) / (1e-4f + sqrt((I.r + I.g) + I.b));
    +inf where n < 2. fault="h_floor": h = n // 2."""
    S = np.asarray(S, dtype=np.float32)
    E = np.asarray(E, dtype=np.float32)
    n = np.broadcast_to(np.asarray(n).astype(np.int64), S.shape[:-1])
    h = n // 2 if fault == "h_floor" else (n + 1) // 2
    with np.errstate(all="ignore"):
        I = S / n.astype(np.float32)[..., None]
        A = E / h.astype(np.float32)[..., None]
        d = np.abs(I - A)
        e = ((d[..., 0] + d[..., 1]) + d[..., 2]) / (np.float32(1e-4) + np.sqrt((I[..., 0] + I[..., 1]) + I[..., 2]))
    return np.where(n < 2, np.float32(np.inf), e).astype(np.float32)


def err_table(S_levels, E_levels, fault=None):
    """err at every level of a ladder: (L + 1, ...) float32."""
    return np.stack([err(S_levels[L], E_levels[L], L, fault=fault) for L in range(len(S_levels))])


def _local_index(N, chunks):
    assert chunks is not None and sum(chunks) >= N
    return np.concatenate([np.arange(c) for c in chunks])[:N]


def unconverged_windows(e, thr, fault):
    """Pixels with some q of their window (3x3 clipped at the border) that is not converged: !(err_q <= thr), NaN included."""
    bad = ~(e < thr) if fault == "lt" else ~(e <= thr)
    r = 2 if fault == "win5" else 1
    h, w = bad.shape
    p = np.pad(bad, r, constant_values=(fault == "border"))
    out = np.zeros_like(bad)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[dy:dy + h, dx:dx + w]
    return out


def err_at(table, n):
    """The err map of a state whose pixel p holds n_p samples: table[n_p][p] (table: per level, an (H, W) err map of that uniform level)."""
    n = np.asarray(n)
    out = np.empty(n.shape, dtype=np.float32)
    for L in np.unique(n):
        m = n == L
        out[m] = np.asarray(table[int(L)], dtype=np.float32)[m]
    return out


def replay(n0, err_of_level, threshold, mn, mx, step, fault=None, err0=None):
    """The adaptive rule on a (H, W) count map n0. err_of_level[L]: the err map at level L (err_at). min 0 = 16, step 0 = 32. err0: the err the
    accumulator holds when the call starts (+inf: fresh, or only uniform renders since creation); only fault="stale" reads it.
    Returns {"samples", "rounds", "added", "error", "progress"}: the final map, the rounds that added samples, their samples, the err the last
    judge saw and the (round, total) progress calls, total = max(round, 1 + ceil((mx - mn) / step))."""
    mn = mn or 16
    step = step or 32
    thr = np.float32(threshold)
    n = np.asarray(n0).astype(np.int64).copy()
    bound = 1 + -(-(mx - mn) // step)
    rounds, added, progress, seen = 0, 0, [], None
    held = np.full(n.shape, np.inf, dtype=np.float32) if err0 is None else np.asarray(err0, dtype=np.float32)
    r = 0
    while True:
        if r == 0:  # round 0: every pixel below min up to it
            t = np.where(n < mn, mn, n)
        else:
            cur = err_at(err_of_level, n)
            seen, held = (held if fault == "stale" else cur), cur  # stale: the judge reads the err the previous judge wrote
            active = (n < mx) & ((n < mn) | unconverged_windows(seen, thr, fault))
            t = np.where(active, n + np.minimum(step, mx - n), n)
        k = t - n
        if k.any():
            rounds += 1
            added += int(k.sum())
            progress.append((rounds, max(rounds, bound)))
            n = t
        elif r > 0:
            break
        r += 1
    return {"samples": n.astype(np.uint32), "rounds": rounds, "added": added, "error": seen, "progress": progress}


def exact_threshold(table, n0, mn, mx, step, q=0.5, need=("lt",), level=None, err0=None):
    """A threshold equal to an err value present at `level` (default: min), the finite value nearest the q-quantile for which the replay under
    each fault of `need` gives another count map than the exact rule: a scenario run at it tells the device apart from those faults."""
    lvl = level if level is not None else (mn or 16)
    e = np.asarray(table[lvl], dtype=np.float32)
    v = np.unique(e[np.isfinite(e)])
    assert len(v), f"no finite err at level {lvl}"
    mid = int(q * (len(v) - 1))
    for i in sorted(range(len(v)), key=lambda i: abs(i - mid))[:400]:
        thr = float(v[i])
        base = replay(n0, table, thr, mn, mx, step, err0=err0)["samples"]
        if all(not np.array_equal(base, replay(n0, table, thr, mn, mx, step, fault=f, err0=err0)["samples"]) for f in need):
            return thr
    raise AssertionError(f"no err value at level {lvl} separates the rule from {need}")


def differs(a, b):
    """Two adaptive outcomes (replays or a device result) that differ in the count map, the rounds or the err of the last judge."""
    return (not np.array_equal(np.asarray(a["samples"]), np.asarray(b["samples"]))) or a["rounds"] != b["rounds"] or not _same(a["error"], b["error"]).all()


# ------------------------------------------------------------------------------------------------ comparisons (raise AssertionError)
def _same(a, b):
    """bit-equal floats, or NaN on both sides (a NaN's payload is the platform's, not the contract's)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _first_bad(ok):
    return tuple(int(i) for i in np.argwhere(~ok)[0])


def assert_floats_equal(got, want, what):
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    ok = _same(got, want)
    if not ok.all():
        i = _first_bad(ok)
        raise AssertionError(f"{what}: {int((~ok).sum())} values differ; first at {i}: got {got[i]!r}, want {want[i]!r}")


def assert_state(state, S, E, n, what=""):
    """An accumulator state (Accumulator.read()) equals the model's S, E (H, W, 3) and n (H, W) bit for bit."""
    got_n = np.asarray(state["samples"])
    ok = got_n == np.asarray(n)
    if not ok.all():
        i = _first_bad(ok)
        raise AssertionError(f"{what} n: {int((~ok).sum())} pixels differ; first at {i}: got {int(got_n[i])}, want {int(np.asarray(n)[i])}")
    assert_floats_equal(state["sum"], S, f"{what} S")
    assert_floats_equal(state["even_sum"], E, f"{what} E")


def assert_replay(got, want, what=""):
    """A device adaptive call against replay(): got = {"samples", "rounds", "added", "error", "progress"} as the device reported them."""
    ok = np.asarray(got["samples"]) == want["samples"]
    if not ok.all():
        i = _first_bad(ok)
        raise AssertionError(f"{what} count map: {int((~ok).sum())} pixels differ; first at {i}: got {int(np.asarray(got['samples'])[i])}, "
                             f"replay {int(want['samples'][i])}")
    for k in ("rounds", "added", "progress"):
        assert got[k] == want[k], f"{what} {k}: got {got[k]}, replay {want[k]}"
    assert_floats_equal(got["error"], want["error"], f"{what} err")
