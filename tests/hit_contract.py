"""The production hit contract, checked per ray and per pixel without a tolerance ("Production modes against the oracle").

A plain module next to the tests (imported like conftest's helpers). Production traversals (global-best pruning, the device-built binary trees,
the 8-wide quantised tree) compute every (b, c, t) with the reference's own triangle test, so a hit they report can be checked exactly:
  * a hit that differs from the oracle's in any word must be reproduced BIT FOR BIT by the oracle's single-object test of the returned index on
    that ray (OracleScene.intersect_objects): a tie resolved to another triangle, a closer hit and a hit where the oracle misses are all real;
  * no hit can be closer than the brute-force minimum over all objects (OracleScene.cast_rays_brute).
`verify_hits` applies that to a batch of rays; `explain_pixels` replays the paths of pixels where a production image differs and requires the
first differing hit of some path to be such a legal hit — a pixel that differs while every ray has the oracle's hit fails (its shading inputs
differ). Both raise AssertionError naming the ray and the three hits (oracle, production, brute force)."""
import contextlib
import importlib
import time

import numpy as np

NONE = 0xFFFFFFFF
BRUTE_SAMPLE_SEED = 0x5EED
# wall time spent inside the checks of this module (outermost calls only), for the report of what they add to a test run
STATS = {"seconds": 0.0, "calls": 0}
_depth = [0]


@contextlib.contextmanager
def _timed():
    _depth[0] += 1
    t0 = time.perf_counter()
    try:
        yield
    finally:
        _depth[0] -= 1
        if _depth[0] == 0:
            STATS["seconds"] += time.perf_counter() - t0
            STATS["calls"] += 1


def _hit_str(p, b):
    if int(p) == NONE:
        return "miss"
    w = np.asarray(b, dtype=np.float32).view(np.uint32)
    return f"({int(p)}, b={float(b[0])!r}, c={float(b[1])!r}, t={float(b[2])!r} [0x{int(w[0]):08x} 0x{int(w[1]):08x} 0x{int(w[2]):08x}])"


def _t_or_inf(p, b):
    return np.where(p == NONE, np.float32(np.inf), b[:, 2]).astype(np.float32)


def verify_reported_hits(orc, rays, gp, gb, idx, what=""):
    """The single-object check alone: for the rays `idx`, the production hit (gp, gb) is reproduced bit for bit by the oracle's test of the object
    it names (an index that names no object, or a miss, fails)."""
    with _timed():
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if not len(idx):
            return 0
        gb = np.ascontiguousarray(gb, dtype=np.float32)
        hit, sb = orc.intersect_objects(np.asarray(rays, dtype=np.float32)[idx], np.asarray(gp, dtype=np.uint32)[idx])
        bad = ~hit | (sb.view(np.uint32) != gb[idx].view(np.uint32)).any(axis=1)
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            i = int(idx[k])
            raise AssertionError(f"{what}: ray {i} {np.asarray(rays)[i].tolist()}: production {_hit_str(gp[i], gb[i])}; the returned object's own test "
                                 f"gives {_hit_str(gp[i], sb[k]) if hit[k] else 'no hit'}: not a hit of that object")
        return len(idx)


def verify_hits(orc, rays, op, ob, gp, gb, kind, brute="all", what="", coplanar_ulps=0):
    """Production hits (gp, gb) on `rays` against the oracle's (op, ob) = orc.cast_rays(rays).

    kind "exact" (global-best pruning, the binary device trees): hit / miss and t bit-equal to the oracle's; only the index may differ.
    kind "superset" (the wide tree): t_brute <= t_prod <= t_oracle, a production miss only where the oracle misses, and t_prod bit-equal to the
    brute-force minimum (the wide tree culls only against its own best t, with boxes that contain the reference's).
    Both: wherever the production hit differs from the oracle's in any word, the single-object test of the returned index reproduces it bit
    for bit; a production miss reports (0, 0, 0).
    brute: "all" = brute force on every ray; an int k = on every ray that differs from the oracle plus a fixed seeded sample of k rays.
    coplanar_ulps (binary device trees on overlapping coplanar triangles only, DESIGN.md "Two kinds of modes"): with kind "exact", a t that
    differs from the oracle's by at most that many ulps is accepted where the index differs and the single-object check passes.
    Returns counts: ties (same t, another triangle or b / c), closer (t below the oracle's), oracle_miss (hit where the oracle misses),
    verified (single-object checks), brute (rays brute-forced), oracle_above_brute (of those, t_oracle > t_brute: the reference's near-local
    pruning skipping a closer triangle; context, not asserted), prod_ne_brute (t_prod differs from t_brute; asserted 0 for "superset")."""
    assert kind in ("exact", "superset"), kind
    with _timed():
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = len(rays)
        op, gp = np.asarray(op, dtype=np.uint32), np.asarray(gp, dtype=np.uint32)
        ob, gb = np.ascontiguousarray(ob, dtype=np.float32), np.ascontiguousarray(gb, dtype=np.float32)
        assert op.shape == gp.shape == (n,) and ob.shape == gb.shape == (n, 3)
        ou, gu = ob.view(np.uint32), gb.view(np.uint32)
        miss_o, miss_g = op == NONE, gp == NONE
        differ = (op != gp) | (ou != gu).any(axis=1)
        brute_hits = {}

        def brute_of(idx):
            missing = [int(i) for i in idx if int(i) not in brute_hits]
            if missing:
                bp, bb = orc.cast_rays_brute(rays[missing])
                for j, i in enumerate(missing):
                    brute_hits[i] = (bp[j], bb[j].copy())
            return brute_hits

        def fail(i, why):
            i = int(i)
            bp, bb = brute_of([i])[i]
            raise AssertionError(f"{what}: ray {i} {rays[i].tolist()}: {why}\n  oracle     {_hit_str(op[i], ob[i])}\n  production {_hit_str(gp[i], gb[i])}\n"
                                 f"  brute force {_hit_str(bp, bb)}")

        # a production miss is (0, 0, 0), as the oracle's
        bad = miss_g & (gu != 0).any(axis=1)
        if bad.any():
            fail(np.flatnonzero(bad)[0], "a production miss with a non-zero (b, c, t)")
        # every production hit that differs from the oracle's is a real hit of the object it names, bit for bit
        chk = np.flatnonzero(differ & ~miss_g)
        if len(chk):
            hit, sb = orc.intersect_objects(rays[chk], gp[chk])
            bad = ~hit | (sb.view(np.uint32) != gu[chk]).any(axis=1)
            if bad.any():
                k = int(np.flatnonzero(bad)[0])
                fail(chk[k], f"the returned object's own test gives {_hit_str(gp[chk[k]], sb[k]) if hit[k] else 'no hit'}: not a hit of that object")
        t_o, t_g = _t_or_inf(op, ob), _t_or_inf(gp, gb)
        if kind == "exact":
            bad = miss_o != miss_g
            if bad.any():
                fail(np.flatnonzero(bad)[0], "hit on one side only")
            bad = t_o.view(np.uint32) != t_g.view(np.uint32)
            if coplanar_ulps:
                ulps = np.abs(t_o.view(np.int32).astype(np.int64) - t_g.view(np.int32).astype(np.int64))
                bad &= (ulps > coplanar_ulps) | (op == gp)
            if bad.any():
                fail(np.flatnonzero(bad)[0], "t differs from the oracle's")
        else:
            bad = miss_g & ~miss_o
            if bad.any():
                fail(np.flatnonzero(bad)[0], "a production miss where the oracle hits")
            bad = t_g > t_o
            if bad.any():
                fail(np.flatnonzero(bad)[0], "a production hit FARTHER than the oracle's")
        # brute force: every ray, or the differing ones plus a fixed sample
        if brute == "all":
            sel = np.arange(n)
        else:
            k = min(int(brute), n)
            sample = np.random.default_rng(BRUTE_SAMPLE_SEED).choice(n, size=k, replace=False) if k else np.zeros(0, dtype=np.int64)
            sel = np.union1d(np.flatnonzero(differ), sample).astype(np.int64)
        bp, bb = (orc.cast_rays_brute(rays[sel]) if len(sel) else (np.zeros(0, np.uint32), np.zeros((0, 3), np.float32)))
        t_b = _t_or_inf(bp, bb)
        t_gs, t_os = t_g[sel], t_o[sel]
        for j in np.flatnonzero(t_gs < t_b)[:1]:
            brute_hits[int(sel[j])] = (bp[j], bb[j].copy())
            fail(sel[j], "a production hit CLOSER than the brute-force minimum over all objects")
        prod_ne_brute = t_gs.view(np.uint32) != t_b.view(np.uint32)
        if kind == "superset":
            for j in np.flatnonzero(prod_ne_brute)[:1]:
                brute_hits[int(sel[j])] = (bp[j], bb[j].copy())
                fail(sel[j], "the wide tree's t is not the brute-force minimum")
        ties = differ & ~miss_o & ~miss_g & (t_o.view(np.uint32) == t_g.view(np.uint32))
        return {
            "rays": n,
            "differ": int(differ.sum()),
            "ties": int(ties.sum()),
            "closer": int((~miss_o & ~miss_g & (t_g < t_o)).sum()),
            "oracle_miss": int((miss_o & ~miss_g).sum()),
            "verified": int(len(chk)),
            "brute": int(len(sel)),
            "oracle_above_brute": int((t_os > t_b).sum()),
            "prod_ne_brute": int(prod_ne_brute.sum()),
        }


def summary(counts):
    """One line of verify_hits counts for the test output."""
    c = counts
    return (f"{c['differ']} of {c['rays']} rays differ from the oracle: {c['ties']} ties, {c['closer']} closer, {c['oracle_miss']} hits where it "
            f"misses, all {c['verified']} verified bit for bit; brute force on {c['brute']}: t_prod != t_brute {c['prod_ne_brute']}, "
            f"t_oracle > t_brute {c['oracle_above_brute']}")


def _packet_contexts(primary):
    """Packets of 64 rays holding `primary` (the bounce-0 rays of one pixel). A packet walks in the octant order of its lane 0, so a tie on a
    primary ray may be resolved by whichever ray leads its packet in the render: the rays are cast in a packet of their own and behind a lead
    ray of each of the eight octants (from the same origin)."""
    o = primary[0, :3]
    leads = [None]
    for oct_ in range(8):
        d = np.array([-1.0 if oct_ & 1 else 1.0, -1.0 if oct_ & 2 else 1.0, -1.0 if oct_ & 4 else 1.0], dtype=np.float32) / np.float32(np.sqrt(3.0))
        leads.append(np.concatenate([o, d]).astype(np.float32))
    batches, idx = [], []
    for lead in leads:
        per = 64 if lead is None else 63
        for s in range(0, len(primary), per):
            chunk = primary[s : s + per]
            pk = chunk if lead is None else np.concatenate([lead[None, :], chunk])
            ix = np.arange(s, s + len(chunk)) if lead is None else np.r_[-1, np.arange(s, s + len(chunk))]
            pad = 64 - len(pk)  # every packet starts at a multiple of 64: fill with copies of its lead
            batches.append(np.concatenate([pk, np.repeat(pk[:1], pad, axis=0)]))
            idx.append(np.r_[ix, np.full(pad, -1)])
    rays = np.concatenate(batches).astype(np.float32)
    idx = np.concatenate(idx).astype(np.int64)
    return rays, idx


def explain_pixels(orc, dev, W, H, spp, seed, pixels, kind, packet=None, global_best=False, brute="all", what="", coplanar_ulps=0, parity=None):
    """Why a production render differs from the oracle (or the parity image, which is the oracle's) in `pixels` ((row, col) pairs).

    The oracle replays each pixel's paths (device-RNG mode, orc.trace_pixel) and logs every ray they cast; the rays go through the production
    scene's own closest-hit kernel (RT_CAST_EXTEND, or RT_CAST_EXTEND_GLOBAL for a global-best render). Up to the first hit that differs from the
    oracle's, a production path IS the oracle's path, so that hit is the cause, and it must be legal: every ray of the pixel goes through
    verify_hits(kind). `packet` (default: spp >= 4, where RT_PACKET_AUTO may walk bounce 0 with the packet kernel): the primary rays are also
    cast through the packet kernel, which may resolve a tie to another triangle than the per-lane kernel. A pixel with no differing ray under
    either kernel fails: the paths met the oracle's hits, so the image differs in what was computed from them.
    The pixel is explained as a whole: one legally differing ray on ANY of its paths suffices, so a shading-input fault confined to a pixel whose
    paths also meet a tie or a closer hit would pass (telling the two apart would take replaying the shading of the diverged paths).
    `parity` (a parity-mode scene, for images compared against the parity render rather than the oracle's): the replayed rays must also give the
    oracle's hits there, bit for bit — the parity image is the oracle's only as far as that holds.
    Returns one record per pixel: the first differing ray, its sample, the kernel and the kind of difference."""
    rt = importlib.import_module("raytracing-course-hw-public_amd")
    mode = rt.RT_CAST_EXTEND_GLOBAL if global_best else rt.RT_CAST_EXTEND
    pmode = rt.RT_CAST_PACKET_GLOBAL if global_best else rt.RT_CAST_PACKET
    if packet is None:
        packet = spp >= 4
    out = []
    with _timed():
        for (y, x) in np.asarray(pixels, dtype=np.int64).reshape(-1, 2):
            y, x = int(y), int(x)
            rays, smp = orc.trace_pixel(W, H, spp, y * W + x, seed=seed)
            op, ob = orc.cast_rays(rays)
            gp, gb = dev.cast_rays_ex(rays, mode)[:2]
            where = f"{what} pixel ({y}, {x})"
            if parity is not None:
                qp_, qb_ = parity.cast_rays_ex(rays, rt.RT_CAST_EXTEND)[:2]
                bad = (qp_ != op) | (qb_.view(np.uint32) != ob.view(np.uint32)).any(axis=1)
                if bad.any():
                    i = int(np.flatnonzero(bad)[0])
                    raise AssertionError(f"{where}: the parity scene's hit on ray {i} is {_hit_str(qp_[i], qb_[i])}, the oracle's {_hit_str(op[i], ob[i])}")
            verify_hits(orc, rays, op, ob, gp, gb, kind, brute=brute, what=f"{where}, per-lane kernel", coplanar_ulps=coplanar_ulps)
            differ = (gp != op) | (gb.view(np.uint32) != ob.view(np.uint32)).any(axis=1)
            first = {}  # sample -> (ray of the pixel, kernel)
            for i in np.flatnonzero(differ):
                first.setdefault(int(smp[i]), (int(i), "per-lane"))
            if packet and len(rays):
                prim_idx = np.flatnonzero(np.r_[True, smp[1:] != smp[:-1]])  # the first ray of every sample: its primary ray
                prays, pidx = _packet_contexts(rays[prim_idx])
                pp, pb = dev.cast_rays_ex(prays, pmode)[:2]
                keep = pidx >= 0
                r = prim_idx[pidx[keep]]
                verify_hits(orc, rays[r], op[r], ob[r], pp[keep], pb[keep], kind, brute=brute, what=f"{where}, packet kernel", coplanar_ulps=coplanar_ulps)
                pdiff = (pp[keep] != op[r]) | (pb[keep].view(np.uint32) != ob[r].view(np.uint32)).any(axis=1)
                for i in r[pdiff]:
                    s = int(smp[i])
                    if s not in first or first[s][0] > int(i):
                        first[s] = (int(i), "packet")
            if not first:
                raise AssertionError(f"{where}: the image differs there, but every ray of its {spp} paths ({len(rays)} rays) has the oracle's hit "
                                     f"under every kernel: the shading inputs differ")
            s = min(first, key=lambda k: first[k][0])
            k, kernel = first[s]
            if kernel == "per-lane":
                qp, qb = gp[k], gb[k]
            else:
                sel = np.flatnonzero((r == k) & pdiff)[0]
                qp, qb = pp[keep][sel], pb[keep][sel]
            if int(op[k]) == NONE:
                cause = "hit where the oracle misses"
            elif qb[2].view(np.uint32) == ob[k, 2].view(np.uint32):
                cause = "exact tie"
            elif qb[2] < ob[k, 2]:
                cause = "closer hit"
            else:
                cause = "coplanar overlap, farther"
            out.append({"pixel": (y, x), "sample": s, "ray_of_pixel": k, "kernel": kernel, "oracle": _hit_str(op[k], ob[k]),
                        "production": _hit_str(qp, qb), "cause": cause})
    return out
