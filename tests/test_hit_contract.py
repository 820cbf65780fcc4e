"""CPU self-tests of tests/hit_contract.py: the checker the production GPU tests rely on must catch one wrong hit, not a share.

The oracle's own results on the five golden fixtures stand in for a production kernel; single faults of the kinds a kernel bug would make (a
wrong triangle index, a barycentric or t one ulp off, a fabricated hit, a pixel that differs while every hit is the oracle's) are injected and
each must raise. The two oracle exports the checker is built on are pinned first: the single-object test reproduces the oracle's own hits bit
for bit, and the brute-force minimum never lies above the oracle's t."""
import numpy as np
import pytest

from conftest import random_rays
from hit_contract import NONE, explain_pixels, verify_hits

FIXTURES = ["room_plain", "room_textured", "open_nolight", "boxes", "room_manylights"]


@pytest.fixture(scope="module")
def cast(oracle, scenes):
    out = {}
    for name in FIXTURES:
        sc = scenes[name]
        orc = oracle.OracleScene(sc)
        rays = random_rays(sc, 20000, seed=31)
        op, ob = orc.cast_rays(rays)
        bp, bb = orc.cast_rays_brute(rays)
        out[name] = (orc, rays, op, ob, bp, bb)
    yield out
    for v in out.values():
        v[0].close()


def _ulp(x, k):
    return np.nextafter(np.float32(x), np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)


@pytest.mark.parametrize("name", FIXTURES)
def test_single_object_test_and_brute_force_agree_with_the_oracle(cast, name):
    orc, rays, op, ob, bp, bb = cast[name]
    h = op != NONE
    hit, sb = orc.intersect_objects(rays[h], op[h])
    assert hit.all() and np.array_equal(sb.view(np.uint32), ob[h].view(np.uint32))
    # no object hit where the oracle misses, and nothing below its t anywhere
    assert np.array_equal(bp == NONE, op == NONE)
    assert (bb[h, 2] <= ob[h, 2]).all()
    # the brute-force hit is a real hit of the object it names
    hb = bp != NONE
    hit, sb = orc.intersect_objects(rays[hb], bp[hb])
    assert hit.all() and np.array_equal(sb.view(np.uint32), bb[hb].view(np.uint32))
    # an index that names no object is no hit
    hit, sb = orc.intersect_objects(rays[:3], np.array([NONE, 10**8, 0], dtype=np.uint32))
    assert not hit[:2].any() and not sb[:2].any()
    # the oracle's own hits pass the exact contract
    c = verify_hits(orc, rays, op, ob, op.copy(), ob.copy(), "exact", what=name)
    assert c["differ"] == 0 and c["brute"] == len(rays) and c["oracle_above_brute"] == 0


def test_brute_force_thread_count_does_not_change_the_result(cast):
    orc, rays, _, _, bp, bb = cast["room_manylights"]
    p1, b1 = orc.cast_rays_brute(rays[:3000], threads=1)
    p3, b3 = orc.cast_rays_brute(rays[:3000], threads=3)
    assert np.array_equal(p1, bp[:3000]) and np.array_equal(p3, p1) and np.array_equal(b1.view(np.uint32), b3.view(np.uint32))


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("kind", ["exact", "superset"])
def test_injected_faults_raise(cast, name, kind):
    orc, rays, op, ob, bp, bb = cast[name]
    hits, misses = np.flatnonzero(op != NONE), np.flatnonzero(op == NONE)
    i = int(hits[len(hits) // 2])

    ties = np.flatnonzero((bp != op) & (bb[:, 2].view(np.uint32) == ob[:, 2].view(np.uint32)) & (op != NONE))

    # 1. a tie's index moved to a neighbouring triangle that is not hit at that t: on a real tie (another triangle at bit-equal t) where the
    #    fixture has one (room_manylights), else on an ordinary hit — the same check fires either way
    i1 = int(ties[0]) if len(ties) else i
    gp, gb = op.copy(), ob.copy()
    for nb in (op[i1] + 1, op[i1] - 1, op[i1] + 2):
        h, sb = orc.intersect_objects(rays[i1 : i1 + 1], np.array([nb], dtype=np.uint32))
        if nb != bp[i1] and not (h[0] and np.array_equal(sb[0].view(np.uint32), ob[i1].view(np.uint32))):
            break
    gp[i1] = nb
    with pytest.raises(AssertionError, match=f"ray {i1} .*not a hit of that object"):
        verify_hits(orc, rays, op, ob, gp, gb, kind, what=name)

    # 2. b one ulp off: on a tied ray where the fixture has one, else on an ordinary hit
    j = int(ties[0]) if len(ties) else i
    gp, gb = op.copy(), ob.copy()
    if len(ties):  # the tie itself resolved to the other triangle is legal
        gp[j], gb[j] = bp[j], bb[j]
        c = verify_hits(orc, rays, op, ob, gp, gb, kind, what=name)
        assert c["ties"] == 1 and c["verified"] == 1 and c["prod_ne_brute"] == 0
    gb[j, 0] = _ulp(gb[j, 0], +1)
    with pytest.raises(AssertionError, match=f"ray {j} .*not a hit of that object"):
        verify_hits(orc, rays, op, ob, gp, gb, kind, what=name)

    # 3. a fabricated hit on a ray the oracle misses (the record of another ray's hit)
    if len(misses):
        m = int(misses[0])
        gp, gb = op.copy(), ob.copy()
        gp[m], gb[m] = op[i], ob[i]
        with pytest.raises(AssertionError, match=f"ray {m} .*not a hit of that object"):
            verify_hits(orc, rays, op, ob, gp, gb, kind, what=name)

    # 4. t one ulp farther, same triangle: no longer that triangle's own hit
    gp, gb = op.copy(), ob.copy()
    gb[i, 2] = _ulp(gb[i, 2], +1)
    with pytest.raises(AssertionError, match=f"ray {i} .*not a hit of that object"):
        verify_hits(orc, rays, op, ob, gp, gb, kind, what=name)

    # 5. t one ulp closer than the brute-force minimum, same triangle: caught first by the single-object check (the brute-force bound itself is
    #    exercised in test_t_contract_branches_fire_on_real_hits, where the single-object check cannot see the fault)
    gp, gb = op.copy(), ob.copy()
    gb[i, 2] = _ulp(bb[i, 2], -1)
    with pytest.raises(AssertionError, match=f"ray {i} .*not a hit of that object"):
        verify_hits(orc, rays, op, ob, gp, gb, kind, brute=0, what=name)


def _farther_real_hit(orc, rays, op, ob, n_tri):
    """A ray the oracle hits that ALSO crosses another triangle farther away: (ray, that triangle, its own (b, c, t)). What a wrongly culled box
    would return — a real hit, just not the closest one."""
    for start in range(0, len(rays), 256):
        cand = np.flatnonzero(op[start : start + 256] != NONE) + start
        if not len(cand):
            continue
        ri = np.repeat(cand, n_tri)
        obj = np.tile(np.arange(n_tri, dtype=np.uint32), len(cand))
        hit, sb = orc.intersect_objects(rays[ri], obj)
        ok = np.flatnonzero(hit & (obj != op[ri]) & (sb[:, 2] > ob[ri, 2]))
        if len(ok):
            k = int(ok[0])
            return int(ri[k]), int(obj[k]), sb[k].copy()
    raise AssertionError("no ray of the fixture crosses two triangles")


@pytest.mark.parametrize("name", FIXTURES)
def test_t_contract_branches_fire_on_real_hits(cast, scenes, name):
    """Faults the single-object check cannot see, because every hit involved is a real hit of the triangle it names; each must be caught by the
    t contract itself, with its own message."""
    orc, rays, op, ob, bp, bb = cast[name]
    i, f, fb = _farther_real_hit(orc, rays, op, ob, scenes[name].n_triangles)
    # a farther triangle's own hit returned instead of the closest one (a box culled wrongly)
    gp, gb = op.copy(), ob.copy()
    gp[i], gb[i] = f, fb
    with pytest.raises(AssertionError, match=f"ray {i} .*t differs from the oracle's"):
        verify_hits(orc, rays, op, ob, gp, gb, "exact", what=name)
    with pytest.raises(AssertionError, match=f"ray {i} .*FARTHER than the oracle's"):
        verify_hits(orc, rays, op, ob, gp, gb, "superset", what=name)
    # the coplanar-overlap allowance of the binary trees (<= 4 ulp, another triangle) does not cover a triangle farther away than that
    if abs(int(fb[2:3].view(np.int32)[0]) - int(ob[i, 2:3].view(np.int32)[0])) > 4:
        with pytest.raises(AssertionError, match=f"ray {i} .*t differs from the oracle's"):
            verify_hits(orc, rays, op, ob, gp, gb, "exact", what=name, coplanar_ulps=4)
    # the same non-minimal real hit as BOTH the oracle's and production's answer: only the brute force can tell, and the superset contract
    # requires t to be the brute-force minimum (the exact contract compares with the oracle only, and counts it)
    with pytest.raises(AssertionError, match=f"ray {i} .*not the brute-force minimum"):
        verify_hits(orc, rays, gp, gb, gp, gb, "superset", what=name)
    c = verify_hits(orc, rays, gp, gb, gp.copy(), gb.copy(), "exact", what=name)
    assert c["differ"] == 0 and c["prod_ne_brute"] == 1 and c["oracle_above_brute"] == 1
    # a fabricated hit one ulp below the brute-force minimum, as both answers: below every object's own hit
    gp, gb = op.copy(), ob.copy()
    gb[i, 2] = _ulp(bb[i, 2], -1)
    for kind in ("exact", "superset"):
        with pytest.raises(AssertionError, match=f"ray {i} .*CLOSER than the brute-force minimum"):
            verify_hits(orc, rays, gp, gb, gp, gb, kind, what=name)
        # ... also where only a seeded sample is brute-forced and the sample holds that ray (it does not differ from the "oracle" here)
        one = slice(i, i + 1)
        with pytest.raises(AssertionError, match="ray 0 .*CLOSER than the brute-force minimum"):
            verify_hits(orc, rays[one], gp[one], gb[one], gp[one], gb[one], kind, brute=1, what=name)
        assert verify_hits(orc, rays[one], gp[one], gb[one], gp[one], gb[one], kind, brute=0, what=name)["brute"] == 0


def test_miss_records_are_checked(cast):
    orc, rays, op, ob, _, _ = cast["boxes"]
    m, h = int(np.flatnonzero(op == NONE)[0]), int(np.flatnonzero(op != NONE)[0])
    gp, gb = op.copy(), ob.copy()
    gb[m, 2] = 1.0  # a miss must report (0, 0, 0)
    for kind in ("exact", "superset"):
        with pytest.raises(AssertionError, match=f"ray {m} .*a production miss with a non-zero"):
            verify_hits(orc, rays, op, ob, gp, gb, kind)
    gp, gb = op.copy(), ob.copy()
    gp[h], gb[h] = NONE, 0.0
    with pytest.raises(AssertionError, match=f"ray {h} .*a production miss where the oracle hits"):
        verify_hits(orc, rays, op, ob, gp, gb, "superset")
    with pytest.raises(AssertionError, match=f"ray {h} .*hit on one side only"):
        verify_hits(orc, rays, op, ob, gp, gb, "exact")


def test_fault_messages_name_the_three_hits(cast):
    orc, rays, op, ob, _, _ = cast["room_plain"]
    gp, gb = op.copy(), ob.copy()
    gb[7, 1] = _ulp(gb[7, 1], -1)
    with pytest.raises(AssertionError) as e:
        verify_hits(orc, rays, op, ob, gp, gb, "superset", what="room_plain")
    msg = str(e.value)
    assert "ray 7 " in msg and "oracle " in msg and "production " in msg and "brute force " in msg


def test_superset_rejects_what_exact_rejects_and_more(cast):
    """A production miss where the oracle hits fails both kinds; a production hit where the oracle misses passes `superset` only as a real hit."""
    orc, rays, op, ob, _, _ = cast["boxes"]
    i = int(np.flatnonzero(op != NONE)[0])
    gp, gb = op.copy(), ob.copy()
    gp[i], gb[i] = NONE, 0.0
    for kind, msg in (("exact", "hit on one side only"), ("superset", "a production miss where the oracle hits")):
        with pytest.raises(AssertionError, match=f"ray {i} .*{msg}"):
            verify_hits(orc, rays, op, ob, gp, gb, kind)
    # the oracle "misses" a ray it hits: production's real hit then passes the superset contract, not the exact one
    mp, mb = op.copy(), ob.copy()
    mp[i], mb[i] = NONE, 0.0
    c = verify_hits(orc, rays, mp, mb, op, ob, "superset")
    assert c["oracle_miss"] == 1 and c["verified"] == 1
    with pytest.raises(AssertionError, match=f"ray {i} .*hit on one side only"):
        verify_hits(orc, rays, mp, mb, op, ob, "exact")


class _OracleAsDevice:
    """Stands in for a production scene: its closest-hit kernels return the oracle's own hits, under every mode."""

    def __init__(self, orc, perturb=None):
        self.orc, self.perturb = orc, perturb

    def cast_rays_ex(self, rays, mode):
        p, b = self.orc.cast_rays(rays)
        if self.perturb is not None:
            p, b = self.perturb(rays, p, b)
        return p, b, {}


@pytest.mark.parametrize("packet", [False, True])
def test_a_differing_pixel_whose_rays_all_have_the_oracles_hit_raises(oracle, scenes, packet):
    """6. Every ray of the pixel's paths has the oracle's hit, yet the image differs there: the shading inputs differ, which no hit explains."""
    orc = oracle.OracleScene(scenes["room_textured"])
    try:
        with pytest.raises(AssertionError, match=r"pixel \(5, 9\).*shading inputs differ"):
            explain_pixels(orc, _OracleAsDevice(orc), 24, 16, 4, 3, [(5, 9)], "superset", packet=packet)
    finally:
        orc.close()


def test_a_differing_pixel_explained_by_a_real_tie(oracle, scenes):
    """The positive case: a pixel whose path meets a tie resolved to the other triangle is explained, and the record names that ray."""
    sc = scenes["room_manylights"]
    orc = oracle.OracleScene(sc)
    try:
        W, H, spp, seed = 40, 30, 2, 9
        found = None
        for pix in range(W * H):  # a pixel one of whose rays has a real tie
            rays, _ = orc.trace_pixel(W, H, spp, pix, seed=seed)
            op, ob = orc.cast_rays(rays)
            bp, bb = orc.cast_rays_brute(rays)
            t = np.flatnonzero((bp != op) & (bb[:, 2].view(np.uint32) == ob[:, 2].view(np.uint32)))
            if len(t):
                found = (pix, int(t[0]))
                break
        if found is None:
            pytest.fail("no tie on any path of the fixture: pick another seed")

        def to_brute(rays, p, b):
            bp, bb = orc.cast_rays_brute(rays)
            return bp, bb

        rec = explain_pixels(orc, _OracleAsDevice(orc, to_brute), W, H, spp, seed, [(found[0] // W, found[0] % W)], "exact", packet=False)
        assert rec[0]["cause"] == "exact tie" and rec[0]["ray_of_pixel"] <= found[1]
        # the same pixel with the tied hit's b one ulp off is not explained
        def bad_b(rays, p, b):
            bp, bb = to_brute(rays, p, b)
            d = np.flatnonzero(bp != p)
            bb[d, 0] = _ulp(bb[d, 0], +1)
            return bp, bb

        with pytest.raises(AssertionError, match="not a hit of that object"):
            explain_pixels(orc, _OracleAsDevice(orc, bad_b), W, H, spp, seed, [(found[0] // W, found[0] % W)], "exact", packet=False)
    finally:
        orc.close()


def test_single_object_test_of_analytic_primitives(oracle, rt):
    """Indices >= n_triangles name the scene-txt primitives (ELLIPSOID / PLANE), reported (0, 0, t): the single-object test and the brute force
    treat them as cast_rays does, and a primitive hit moved to another primitive is caught."""
    import os

    ls = rt.parse_scene_txt(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "txt", "cornell_mixed.txt"))
    n_tri = ls.arrays()["positions"].reshape(-1, 9).shape[0]
    orc = oracle.OracleScene(ls)
    try:
        cam = ls.arrays()["camera"]["position"]
        d = np.random.default_rng(5).normal(size=(4000, 3)).astype(np.float32)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.concatenate([np.tile(cam, (4000, 1)), d], axis=1).astype(np.float32)
        op, ob = orc.cast_rays(rays)
        bp, bb = orc.cast_rays_brute(rays)
        assert np.array_equal(op, bp) and np.array_equal(ob.view(np.uint32), bb.view(np.uint32))
        prim = np.flatnonzero((op != NONE) & (op >= n_tri))
        assert len(prim) > 100
        hit, sb = orc.intersect_objects(rays[prim], op[prim])
        assert hit.all() and np.array_equal(sb.view(np.uint32), ob[prim].view(np.uint32)) and not sb[:, :2].any()
        gp = op.copy()
        i = int(prim[0])
        gp[i] = n_tri + (op[i] - n_tri + 1) % (len(ls.arrays()["primitives"]) or 1)
        for kind in ("exact", "superset"):
            with pytest.raises(AssertionError, match=f"ray {i} "):
                verify_hits(orc, rays, op, ob, gp, ob, kind)
    finally:
        orc.close()
