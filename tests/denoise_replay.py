"""A host model of rt_accum_denoise (include/rt_abi.h, "The rule, exactly"), in numpy float32: one float32 operation for each operation the
header states, in the header's order. Vectorised over the pixels; sequential over the 3x3 window of the noise scale and over the 25 taps,
dy outer, dx inner. A plain module next to the tests (imported like adaptive_replay.py).
`fault=` selects a variant a subtly wrong kernel would follow (FAULTS); the CPU tests require each of them to change the output of some case,
so a GPU test that compares the device with the exact model bit for bit and passes has ruled each of them out."""
import numpy as np

FAULTS = ("tap_order", "stride", "no_centre", "no_wz", "window")  # taps visited in reverse; stride 1 in every iteration; the centre tap left
                                                                  # out; wz = 1; the 3x3 window of s_p divided by 9 instead of its valid pixels
F = np.float32
K = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))
DEFAULTS = dict(iterations=5, sigma_color=8.0, sigma_depth=0.5, normal_sharpness=3)


def _shift(a, ox, oy, fill):
    """out[y, x] = a[y + oy, x + ox] where that lies inside the image, `fill` elsewhere."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys0, ys1 = max(0, -oy), min(h, h - oy)
    xs0, xs1 = max(0, -ox), min(w, w - ox)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = a[ys0 + oy:ys1 + oy, xs0 + ox:xs1 + ox]
    return out


def prepare(S, E, n, AS, NS, ZS, hits, demodulate=True, fault=None):
    """The per-pixel terms: valid, hit (H, W) bool; C, den, L0, N (H, W, 3); Z, s (H, W), all float32."""
    S, E, AS, NS = (np.asarray(a, dtype=F) for a in (S, E, AS, NS))
    ZS = np.asarray(ZS, dtype=F)
    n = np.asarray(n).astype(np.int64)
    hits = np.asarray(hits).astype(np.int64)
    valid, hit = n > 0, hits > 0
    with np.errstate(all="ignore"):
        fn = n.astype(F)
        C = S / fn[..., None]
        if demodulate:
            alb = AS / fn[..., None]
            m = (n - hits).astype(F) / fn
            den = (alb + m[..., None]) + F(1e-3)
        else:
            den = np.ones_like(C)
        L0 = C / den
        N = NS / fn[..., None]
        Z = np.where(hit, ZS / hits.astype(F), F(0)).astype(F)
        A = E / ((n + 1) // 2).astype(F)[..., None]
        d = np.abs(C - A) / den
        d = (d[..., 0] + d[..., 1]) + d[..., 2]
        d = np.where(n < 2, F(np.inf), d).astype(F)
        tot = np.zeros(n.shape, dtype=F)
        cnt = np.zeros(n.shape, dtype=np.int64)
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                vq = _shift(valid, ox, oy, False)
                dq = _shift(d, ox, oy, F(0))
                tot = np.where(vq, tot + dq, tot)
                cnt += 1 if fault == "window" else vq
        s = tot / cnt.astype(F)
    z3 = np.zeros_like(C)
    return dict(valid=valid, hit=hit, C=np.where(valid[..., None], C, z3), den=np.where(valid[..., None], den, z3), L0=np.where(valid[..., None], L0, z3),
                N=np.where(valid[..., None], N, z3), Z=np.where(valid, Z, F(0)), s=np.where(valid, s, F(0)).astype(F))


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def iterate(P, L, i, sigma_color, sigma_depth, normal_sharpness, fault=None):
    """One iteration (index i, stride 2^i) over the working signal L (H, W, 3)."""
    t = 1 if fault == "stride" else 1 << i
    valid, hit, N, Z, s = P["valid"], P["hit"], P["N"], P["Z"], P["s"]
    with np.errstate(all="ignore"):
        cden = (F(sigma_color) * s) * (F(1) / F(t)) + F(1e-6)
        pp = _dot(N, N)
        sw = np.zeros(valid.shape, dtype=F)
        acc = np.zeros(L.shape, dtype=F)
        taps = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3)]
        if fault == "tap_order":
            taps.reverse()
        for dx, dy in taps:
            centre = dx == 0 and dy == 0
            if centre and fault == "no_centre":
                continue
            vq = _shift(valid, t * dx, t * dy, False)
            Lq = _shift(L, t * dx, t * dy, F(0))
            w = np.full(valid.shape, K[dy + 2] * K[dx + 2], dtype=F)
            if not centre:
                Nq = _shift(N, t * dx, t * dy, F(0))
                Zq = _shift(Z, t * dx, t * dy, F(0))
                hq = _shift(hit, t * dx, t * dy, False)
                a, qq = _dot(N, Nq), _dot(Nq, Nq)
                pq = pp * qq
                c = (a * a) / pq
                for _ in range(int(normal_sharpness)):
                    c = c * c
                wn = np.where((pp == 0) & (qq == 0), F(1), np.where((a <= 0) | (pq == 0), F(0), c)).astype(F)
                r = (Z - Zq) / ((F(sigma_depth) * F(t * max(abs(dx), abs(dy)))) * np.maximum(Z, Zq))
                wz = np.where(~hit & ~hq, F(1), np.where(hit != hq, F(0), F(1) / (F(1) + r * r))).astype(F)
                if fault == "no_wz":
                    wz = np.ones_like(wz)
                dL = np.abs(L - Lq)
                e = ((dL[..., 0] + dL[..., 1]) + dL[..., 2]) / cden
                wc = F(1) / (F(1) + e * e)
                w = ((w * wn) * wz) * wc
            sw = np.where(vq, sw + w, sw)
            acc = np.where(vq[..., None], acc + w[..., None] * Lq, acc)
        out = acc / sw[..., None]
    return np.where(valid[..., None], out, F(0)).astype(F)


def denoise(S, E, n, AS, NS, ZS, hits, iterations=0, sigma_color=0.0, sigma_depth=0.0, normal_sharpness=0, demodulate=True, fault=None):
    """rt_accum_denoise of an accumulator state (Accumulator.read() and read_features()): (H, W, 3) float32. 0 = the default, as in rt_denoise."""
    K_it = iterations or DEFAULTS["iterations"]
    sc = sigma_color or DEFAULTS["sigma_color"]
    sd = sigma_depth or DEFAULTS["sigma_depth"]
    sh = normal_sharpness or DEFAULTS["normal_sharpness"]
    P = prepare(S, E, n, AS, NS, ZS, hits, demodulate=demodulate, fault=fault)
    L = P["L0"]
    for i in range(K_it):
        L = iterate(P, L, i, sc, sd, sh, fault=fault)
    return np.where(P["valid"][..., None], L * P["den"], F(0)).astype(F)


def of_accumulator(acc, **opts):
    """The model fed with an accumulator's own read-back state."""
    r, f = acc.read(), acc.read_features()
    return denoise(r["sum"], r["even_sum"], r["samples"], f["albedo_sum"], f["normal_sum"], f["depth_sum"], f["hits"], **opts)


def rel_mse(x, ref):
    """mean((x - ref)^2 / (ref^2 + 1e-2)) in float64."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))
