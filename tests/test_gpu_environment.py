"""GPU tests of the float environment (include/rt_abi.h rt_set_environment): the lookup, the distribution's tables, pdf and sampler against
the numpy restatement (tests/env_replay.py), the exact identities the new shading branch must keep, the statistics that show the estimator
unbiased and worth having, and the refusals."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import env_replay as er

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = os.path.join(HERE, "golden", "envmap")
W, H = 64, 48
EPS = 2.0 ** -24
K, SPP_LONG = 8, 2048
INVALID, UNSUPPORTED = 1, 8


def float_map(seed=7, w=64, h=32):
    """High dynamic range, every texel comfortably positive (no cell falls below the float spacing of its table)."""
    r = np.random.default_rng(seed).random((h, w, 3))
    return (0.01 + 30.0 * r ** 6).astype(np.float32)


def refused(fn, code):
    with pytest.raises(Exception) as e:
        fn()
    assert getattr(e.value, "code", None) == code, e.value
    return True


@pytest.fixture(scope="module")
def long_renders(gpu, scenes):
    """K renders of SPP_LONG samples with different seeds, with and without RT_ENV_IMPORTANCE, of the sky with a 2 x 2 texel sun of ~1e3 over
    open_nolight (mix_dist = {cosine, env}) and boxes ({cosine, lights, env}): made once, shared by the unbiasedness and the variance tests."""
    out = {}
    for name in ("open_nolight", "boxes"):
        dev = gpu.DeviceScene(scenes[name])
        try:
            for flag in (False, True):
                dev.set_environment(er.sky(), importance=flag)
                out[name, flag] = np.stack([dev.run_raytracer(W, H, SPP_LONG, seed=(100 if flag else 0) + k + 1)[0] for k in range(K)])
        finally:
            dev.close()
    return out


# ------------------------------------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("name", ["open_nolight", "boxes"])
def test_1x1_map_is_a_scaled_background_bit_for_bit(gpu, scenes, name):
    sc = copy.copy(scenes[name])
    sc.bg_color = (0.5, 0.75, 1.25)
    c = np.array([0.7, 1.3, 2.5], dtype=np.float32)
    scaled = copy.copy(sc)
    scaled.bg_color = tuple(float(x) for x in np.array(sc.bg_color, dtype=np.float32) * c)
    dev, ref = gpu.DeviceScene(sc), gpu.DeviceScene(scaled)
    try:
        dev.set_environment(c.reshape(1, 1, 3))
        a, _ = dev.run_raytracer(W, H, 4, seed=3)
        b, _ = ref.run_raytracer(W, H, 4, seed=3)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        d = np.random.default_rng(1).normal(size=(64, 3)).astype(np.float32)
        assert np.array_equal(dev.bg_at(d).view(np.uint32), ref.bg_at(d).view(np.uint32))
    finally:
        dev.close()
        ref.close()


@pytest.mark.parametrize("with_texture", [False, True])
def test_null_environment_restores_every_bit(gpu, scenes, with_texture):
    sc = copy.copy(scenes["open_nolight"])
    if with_texture:
        sc.textures = list(sc.textures) + [gpu.image_decode(os.path.join(ENV, "env.png"))]
        sc.bg_texture = len(sc.textures) - 1
    d = np.load(os.path.join(ENV, "expected.npz"))["dirs"][:512]
    dev = gpu.DeviceScene(sc)
    try:
        fb0, _ = dev.run_raytracer(W, H, 4, seed=9)
        bg0 = dev.bg_at(d)
        mega0, _ = dev.run_raytracer(W, H, 2, seed=9, megakernel=True)
        dev.set_environment(float_map(), importance=True)
        fb1, _ = dev.run_raytracer(W, H, 4, seed=9)
        assert not np.array_equal(fb1, fb0)  # the map is really used
        dev.set_environment(None)
        fb2, _ = dev.run_raytracer(W, H, 4, seed=9)
        assert np.array_equal(fb2.view(np.uint32), fb0.view(np.uint32))
        assert np.array_equal(dev.bg_at(d).view(np.uint32), bg0.view(np.uint32))
        mega2, _ = dev.run_raytracer(W, H, 2, seed=9, megakernel=True)  # the parity entry points are back as well
        assert np.array_equal(mega2.view(np.uint32), mega0.view(np.uint32))
    finally:
        dev.close()


def test_update_geometry_leaves_the_environment(gpu, scenes):
    dev = gpu.DeviceScene(scenes["boxes"])
    try:
        dev.set_environment(er.sky(), importance=True)
        a, _ = dev.run_raytracer(W, H, 4, seed=2)
        dev.update_geometry(scenes["boxes"])
        b, _ = dev.run_raytracer(W, H, 4, seed=2)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------------------------------------ 2. lookup
def test_bg_at_is_the_float_bilinear_lookup(gpu, scenes):
    """rt_bg_at against the float64 bilinear replay at the fixture's directions. The bound, derived: the device's (u, v) carry atan2f / asinf
    (<= 1 ulp each), one division and the final rounding to float, so |du|, |dv| <= 4 eps (eps = 2^-24, u, v <= 1); tx = u * W adds half an
    ulp of tx <= W eps / 2, so the blend weights are off by at most ddx = 5 W eps and ddy = 5 H eps. A bilinear blend moves by at most
    (ddx + ddy) * R when its weights move, R = the spread of the footprint's four texels; its own arithmetic (3 products and 2 sums per lerp
    level, then bg *) rounds at most 8 times: 8 eps relative. So |got - want| <= bg * (5 (W + H) eps * R) + 8 eps * |want| per component.
    Directions within 1e-4 texels of a texel edge may take the neighbouring footprint on the device and are skipped (at most 1 %)."""
    tex, bg = float_map(), (0.5, 1.0, 2.0)
    sc = copy.copy(scenes["open_nolight"])
    sc.bg_color = bg
    d = np.load(os.path.join(ENV, "expected.npz"))["dirs"]
    dev = gpu.DeviceScene(sc)
    try:
        dev.set_environment(tex)
        got = dev.bg_at(d).astype(np.float64)
    finally:
        dev.close()
    want, ok, (x0, y0, x1, y1, dx, dy) = er.radiance64(tex, bg, d)
    assert ok.sum() >= 3000  # NaN (u, v) (|y| > 1: the fixture's directions are not all unit length) are skipped, as NaN never compares
    edge = np.minimum(np.minimum(dx, 1 - dx), np.minimum(dy, 1 - dy)) <= 1e-4
    assert (edge & ok).sum() <= 0.01 * ok.sum(), int((edge & ok).sum())
    use = ok & ~edge
    t64 = tex.astype(np.float64)
    foot = np.stack([t64[y0, x0], t64[y1, x0], t64[y0, x1], t64[y1, x1]])
    spread = foot.max(axis=0) - foot.min(axis=0)
    th, tw = tex.shape[:2]
    tol = np.array(bg) * (5.0 * (tw + th) * EPS * spread) + 8.0 * EPS * np.abs(want)
    err = np.abs(got - want)
    print("lookup: worst error / bound =", float((err[use] / np.maximum(tol[use], 1e-300)).max()))
    assert (err[use] <= tol[use]).all()


# ------------------------------------------------------------------------------------------------------------------------------ 3. pdf and sample
@pytest.fixture(scope="module")
def dist_scene(gpu, scenes):
    tex, bg = float_map(11), (1.0, 0.8, 1.2)
    sc = copy.copy(scenes["open_nolight"])
    sc.bg_color = bg
    dev = gpu.DeviceScene(sc)
    dev.set_environment(tex, importance=True)
    yield dev, er.Tables(tex, bg)
    dev.close()


def pdf_probe_points(t):
    """Every cell centre, then 1e4 random directions at least 1e-2 texels inside their cell"""
    d = np.random.default_rng(5).normal(size=(40000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    _, _, edge = er.cell_of(d, t.W, t.H)
    d = np.concatenate([er.cell_centres(t.W, t.H), d[edge > 1e-2][:10000]])
    assert len(d) == t.W * t.H + 10000
    return d


def test_env_pdf_equals_the_replay(gpu, scenes, dist_scene):
    """pdf at every cell centre and at 1e4 interior points: the replay's value for the replay's cell to 1e-5 relative, on a map of high
    dynamic range. The probe returns no index, so the index is checked through the value on a second map, a ramp whose footprint maxima
    differ from cell to cell: at the points whose eight neighbouring cells all hold a pdf more than 1e-3 away (relative), a match to 1e-5
    can only be the same cell. (The ramp's wrap-around column and row tie with their neighbours: those points check the value alone.)"""
    dev, t = dist_scene
    d = pdf_probe_points(t)
    i, j, _ = er.cell_of(d, t.W, t.H)
    want = t.pdf_cells[i, j].astype(np.float64)
    got = dev.env_pdf(d.astype(np.float32)).astype(np.float64)
    rel = np.abs(got - want) / want
    print("env_pdf: worst relative error", float(rel.max()))
    assert (want > 0).all() and (rel <= 1e-5).all()

    y, x = np.mgrid[0:16, 0:32]
    ramp = (((1.0 + y * 32 + x) ** 2)[..., None] * np.ones(3)).astype(np.float32)
    t = er.Tables(ramp)
    d = pdf_probe_points(t)
    i, j, _ = er.cell_of(d, t.W, t.H)
    want = t.pdf_cells[i, j].astype(np.float64)
    distinct = np.ones(len(d), dtype=bool)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            if di or dj:
                ii = np.clip(i + di, 0, t.H - 1)
                nb = t.pdf_cells[ii, (j + dj) % t.W].astype(np.float64)
                distinct &= (np.abs(nb - want) > 1e-3 * want) | ((ii == i) & (dj == 0))
    assert distinct.mean() > 0.75
    ramp_dev = gpu.DeviceScene(scenes["open_nolight"])
    try:
        ramp_dev.set_environment(ramp, importance=True)
        got = ramp_dev.env_pdf(d.astype(np.float32)).astype(np.float64)
    finally:
        ramp_dev.close()
    assert (np.abs(got - want) <= 1e-5 * want).all()


def test_env_sample_lands_in_the_replay_cells(gpu, dist_scene):
    dev, t = dist_scene
    n = 1000000
    xi = np.random.default_rng(20261019).random((n, 4), dtype=np.float32)
    d = dev.env_sample(xi)
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    wi, wj = er.select(t, xi)
    gi, gj, _ = er.cell_of(d, t.W, t.H)
    same = (gi == wi) & (gj == wj)
    print("env_sample: fraction in the replay's cell", float(same.mean()))
    assert same.mean() >= 0.999
    ddj = np.abs(gj - wj)
    assert (np.abs(gi - wi)[~same] <= 1).all() and (np.minimum(ddj, t.W - ddj)[~same] <= 1).all()  # the rest: neighbours, at table or float boundaries
    ok, worst = er.histogram_ok(gi, gj, t.p, n)  # the device's own samples follow p_ij
    print("env_sample: worst histogram deviation / bound", worst)
    assert ok, worst
    assert (dev.env_pdf(d) > 0).all()
    rep, _, _ = er.sample(t, xi[:4096])
    assert np.abs(rep.astype(np.float64) - d[:4096]).max() < 1e-5  # the same direction, up to numpy's sinf / cosf


# ------------------------------------------------------------------------------------------------------------------------------ 4. unbiased
@pytest.mark.parametrize("name", ["open_nolight", "boxes"])
def test_importance_sampling_is_unbiased(long_renders, name):
    """Two-sample test, no fixed tolerance: per 16 x 16 pixel block the means of the flagged and the unflagged renders differ by at most 5
    standard errors of the difference, the standard errors estimated from the spread of the K renders on each side."""
    a, b = long_renders[name, False], long_renders[name, True]
    assert a.shape == (K, H, W, 3)
    blocks = lambda x: x.astype(np.float64).reshape(K, 3, H // 3, 4, W // 4, 3).mean(axis=(2, 4, 5))  # (K, 3, 4)
    ma, mb = blocks(a), blocks(b)
    se = np.sqrt(ma.var(axis=0, ddof=1) / K + mb.var(axis=0, ddof=1) / K)
    z = np.abs(ma.mean(axis=0) - mb.mean(axis=0)) / se
    print(name, "block z-scores:", np.round(z, 2).tolist())
    assert (z <= 5.0).all()
    assert not np.array_equal(a[0], b[0])


# ------------------------------------------------------------------------------------------------------------------------------ 5. worth having
def test_importance_sampling_lowers_the_error(gpu, scenes, long_renders):
    ref = long_renders["open_nolight", False].astype(np.float64).mean(axis=0)  # 16 384 SPP without the flag
    dev = gpu.DeviceScene(scenes["open_nolight"])
    try:
        rmse = {}
        for flag in (False, True):
            dev.set_environment(er.sky(), importance=flag)
            fb, _ = dev.run_raytracer(W, H, 64, seed=77)
            rmse[flag] = float(np.sqrt(((fb.astype(np.float64) - ref) ** 2).mean()))
    finally:
        dev.close()
    print("RMSE at 64 SPP: without the flag", rmse[False], "with it", rmse[True], "ratio", rmse[True] / rmse[False])
    assert rmse[True] < rmse[False]


# ------------------------------------------------------------------------------------------------------------------------------ 6. everywhere
@pytest.mark.parametrize("name", ["open_nolight", "boxes"])
def test_every_entry_point_shades_the_same(gpu, scenes, name):
    sc = scenes[name]
    dev = gpu.DeviceScene(sc)
    try:
        dev.set_environment(er.sky(), importance=True)
        fb, st = dev.run_raytracer(W, H, 8, seed=21, counters=True)
        plain, _ = dev.run_raytracer(W, H, 8, seed=21)
        assert np.array_equal(fb.view(np.uint32), plain.view(np.uint32))  # the RT_FLAG_COUNTERS variant equals the plain one
        assert st["samples"] == W * H * 8
        views, _ = dev.run_raytracer_views(W, H, 8, [sc.camera], [21])
        assert np.array_equal(views[0].view(np.uint32), fb.view(np.uint32))
        sens, _ = dev.render_sensors(W, H, 8, [gpu.Sensor.pinhole(sc.camera, seed=21)])
        assert np.array_equal(sens[0].view(np.uint32), fb.view(np.uint32))
        small, _ = dev.run_raytracer(W, H, 8, seed=21, max_paths=4096, sort_mode=gpu.RT_SORT_OFF)  # scheduling changes no bit
        assert np.array_equal(small.view(np.uint32), fb.view(np.uint32))
        acc = dev.accumulator(W, H, seed=21)
        acc.render(3)
        acc.render(5)
        assert np.array_equal(acc.image().view(np.uint32), fb.view(np.uint32))
        # an accumulator's sums are of the environment it was made under: the scene refuses a change while one lives
        assert refused(lambda: dev.set_environment(None), INVALID)
        assert refused(lambda: dev.set_environment(er.sky()), INVALID)
        acc.close()
        dev.set_environment(None)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(gpu, scenes):
    sc = scenes["boxes"]
    dev = gpu.DeviceScene(sc)
    try:
        ok = np.ones((4, 8, 3), dtype=np.float32)
        assert refused(lambda: dev.env_pdf(np.zeros((1, 3), dtype=np.float32)), INVALID)  # no environment yet
        for shape in ((1, 0, 3), (0, 1, 3), (1, 8193, 3), (4097, 1, 3)):  # bad sizes
            assert refused(lambda: dev.set_environment(np.ones(shape, dtype=np.float32)), INVALID)
        for bad in (np.nan, np.inf, -1.0):
            m = ok.copy()
            m[2, 5, 1] = bad
            assert refused(lambda: dev.set_environment(m), INVALID)

        def raw(flags, reserved):
            e = gpu.RtEnvironment()
            e.height, e.width, e.rgb, e.flags, e.reserved = 4, 8, ok.ctypes.data_as(C.POINTER(C.c_float)), flags, reserved
            gpu._check(gpu.lib().rt_set_environment(dev._h, C.byref(e)))

        assert refused(lambda: raw(2, 0), INVALID)  # unknown flag
        assert refused(lambda: raw(1, 1), INVALID)  # reserved
        fb0, _ = dev.run_raytracer(W, H, 2, seed=1)  # nothing above changed the scene
        dev.set_environment(er.sky(), importance=True)
        assert refused(lambda: dev.run_raytracer(W, H, 2, megakernel=True), UNSUPPORTED)
        assert refused(lambda: dev.run_raytracer(W, H, 2, rng_mode=gpu.RT_RNG_REFERENCE), UNSUPPORTED)
        assert refused(lambda: dev.env_sample(np.array([[0.5, 0.5, 1.0, 0.5]], dtype=np.float32)), INVALID)
        assert refused(lambda: dev.set_environment(ok * np.float32(np.nan)), INVALID)
        fb1, _ = dev.run_raytracer(W, H, 2, seed=1)  # a refusal leaves the environment that was set
        assert not np.array_equal(fb1, fb0)
        # an all-zero map has no distribution: the flag acts as if it were not set
        zero = np.zeros((4, 8, 3), dtype=np.float32)
        dev.set_environment(zero, importance=True)
        a, _ = dev.run_raytracer(W, H, 4, seed=6)
        assert refused(lambda: dev.env_pdf(np.zeros((1, 3), dtype=np.float32)), INVALID)
        dev.set_environment(zero)
        b, _ = dev.run_raytracer(W, H, 4, seed=6)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    finally:
        dev.close()
    grp = gpu.DeviceScene(sc, device=[0, 0], build_flags=gpu.RT_BUILD_GROUP_COPY)
    try:
        assert refused(lambda: grp.set_environment(er.sky()), UNSUPPORTED)
    finally:
        grp.close()
