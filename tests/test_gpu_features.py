"""First-hit feature sums of a feature accumulator (include/rt_abi.h, RT_ACCUM_FEATURES), pinned bit for bit: ZS, h against the oracle's
closest hits of the primary rays, AS against the oracle's samples of the twin scene (feature_replay.twin_scene), NS against the
rt_surface_normals probe folded on the host and, on flat-shaded triangles, against a float64 evaluation; under every schedule, after every
split of the samples over calls, and without moving anything an accumulator had before."""
import numpy as np
import pytest

import feature_replay as fr
import hit_contract

pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 8
SEED = 7
COUNTERS = ("samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests",
            "light_tri_tests", "light_hits", "texel_fetches")


class _Case:
    """One scene at one image size: the model's ladders of the four sums, levels 0 .. n. `sc` None: a loaded scene without a twin (no albedo)."""

    def __init__(self, dev, orc, oracle, sc, w=W, h=H, n=N, seed=SEED):
        self.dev, self.orc, self.sc, self.w, self.h, self.n, self.seed = dev, orc, sc, w, h, n, seed
        self.rays = fr.primary_rays(orc, w, h, n, seed)
        self.hit, self.t, self.prim = fr.first_hits(orc, self.rays)
        self.Z, self.Hn = fr.ladder(self.t), fr.hit_ladder(self.hit)
        self.A = None
        if sc is not None:
            # the twin's precondition, checked on the CPU: colour alpha is 1 in the twin's materials by construction and in every colour texel
            assert fr.twin_alpha_is_one(sc)
            tw = oracle.OracleScene(fr.twin_scene(sc))
            self.A = fr.ladder(tw.pixel_samples(w, h, n, np.arange(w * h), seed=seed))
            tw.close()
        # the shading normals of the same rays through the probe kernel (another kernel over the same make_surf)
        pp, pt, _, sn = dev.surface_normals(self.rays.reshape(-1, 6))
        self.probe_t = pt.reshape(w * h, n)
        self.sn = sn.reshape(w * h, n, 3)
        self.NS = fr.ladder(self.sn)

    def check(self, acc, what, albedo=True, normals=True):
        n = acc.read()["samples"]
        f = acc.read_features()
        shape = (self.h, self.w)
        assert np.array_equal(f["hits"], fr.at(self.Hn, n).reshape(shape)), f"{what}: h"
        fr.assert_bits(f["depth_sum"], fr.at(self.Z, n), f"{what}: ZS")
        if albedo and self.A is not None:
            fr.assert_bits(f["albedo_sum"], fr.at(self.A, n), f"{what}: AS")
        if normals:
            fr.assert_bits(f["normal_sum"], fr.at(self.NS, n), f"{what}: NS")
        return n, f


def _case(gpu, oracle, scenes, name, **kw):
    dev, orc = gpu.DeviceScene(scenes[name]), oracle.OracleScene(scenes[name])
    return _Case(dev, orc, oracle, scenes[name], **kw)


@pytest.fixture(scope="module")
def plain(gpu, oracle, scenes):
    c = _case(gpu, oracle, scenes, "room_plain")
    yield c
    c.dev.close()
    c.orc.close()


@pytest.fixture(scope="module")
def textured(gpu, oracle, scenes):
    c = _case(gpu, oracle, scenes, "room_textured")
    yield c
    c.dev.close()
    c.orc.close()


def _split_renders(case, what, **kw):
    acc = case.dev.accumulator(case.w, case.h, seed=case.seed, features=True)
    total = 0
    for k in (1, 2, 5):  # the calls start at bases 0, 1 and 3
        acc.render(k)
        total += k
        n, _ = case.check(acc, f"{what} after {total}", **kw)
        assert np.all(n == total)
    acc.close()


# ------------------------------------------------------------------------------------------------ 1: depth, hits
def test_depth_and_hits_room_plain(plain):
    assert plain.hit.all()
    _split_renders(plain, "room_plain")


def test_depth_and_hits_open_scene_with_misses(gpu, oracle, scenes):
    c = _case(gpu, oracle, scenes, "open_nolight")
    assert c.hit.any() and (~c.hit).any()
    _split_renders(c, "open_nolight")
    c.dev.close()
    c.orc.close()


def test_depth_and_hits_analytic_primitives(gpu, oracle):
    from conftest import SCENE000

    ls = gpu.parse_scene_txt(SCENE000)
    dev, orc = gpu.DeviceScene(ls), oracle.OracleScene(ls)
    c = _Case(dev, orc, oracle, None)
    assert (c.prim == 12).any() and (c.prim == 13).any()  # the ELLIPSOID and the PLANE win primary rays
    _split_renders(c, "scene-000.txt")
    # an analytic primitive's shading normal is its normal: the probe's two normals agree on those rays
    _, _, gn, sn = dev.surface_normals(c.rays.reshape(-1, 6))
    on_prim = (c.prim >= 12).reshape(-1) & c.hit.reshape(-1)
    assert fr.same_bits(gn[on_prim], sn[on_prim])
    dev.close()
    orc.close()


# ------------------------------------------------------------------------------------------------ 2: albedo
def test_albedo_untextured(plain):
    mats = np.array([m.color[:3] for m in plain.sc.materials], np.float32)
    want = mats[plain.sc.material_ids[plain.prim]]
    assert fr.same_bits(plain.A[1], want[:, 0])  # the twin's first sample IS the hit triangle's material colour
    acc = plain.dev.accumulator(W, H, seed=SEED, features=True)
    acc.render(3)
    acc.render(5)
    plain.check(acc, "room_plain albedo")
    acc.close()


def test_albedo_textured(textured):
    assert any(m.color_tex >= 0 for m in textured.sc.materials)
    # the fixture's primary rays mostly see the untextured walls; enough of them land on textured triangles that the albedos are texels (more
    # distinct values than there are materials), not a handful of material colours
    on_tex = np.array([m.color_tex >= 0 for m in textured.sc.materials])[textured.sc.material_ids[textured.prim]]
    distinct = len(np.unique(textured.A[1].view(np.uint32), axis=0))
    print(f"room_textured: {int(on_tex.sum())} of {on_tex.size} primary rays hit textured triangles; {distinct} distinct first-sample albedos")
    assert on_tex.sum() >= 50 and distinct > len(textured.sc.materials)
    _split_renders(textured, "room_textured")


# ------------------------------------------------------------------------------------------------ 3: normals
def test_normals_flat_shaded_against_float64(plain):
    assert plain.sc.normals is None and not plain.sc.textures
    assert fr.same_bits(plain.probe_t, plain.t)
    acc = plain.dev.accumulator(W, H, seed=SEED, features=True)
    acc.render(N)
    plain.check(acc, "room_plain normals")
    mean = acc.features()["normal"].reshape(-1, 3)
    g = fr.geometric_normals_f64(plain.sc, plain.rays, plain.prim, plain.hit)
    want = g.sum(axis=1) / N
    err = np.abs(mean.astype(np.float64) - want).max()
    print(f"mean normal vs float64: max abs error {err:.3e}")
    assert err <= 1e-6
    acc.close()


def test_feature_means(textured):
    acc = textured.dev.accumulator(W, H, seed=SEED, features=True)
    acc.render(3)
    acc.render_adaptive(0.05, min_samples=4, max_samples=N, step=2)
    n, f = textured.check(acc, "means")
    m = acc.features()
    fn = n.astype(np.float32)
    fr.assert_bits(m["albedo"], f["albedo_sum"] / fn[..., None], "albedo mean")
    fr.assert_bits(m["normal"], f["normal_sum"] / fn[..., None], "normal mean")
    with np.errstate(all="ignore"):
        z = np.where(f["hits"] > 0, f["depth_sum"] / f["hits"].astype(np.float32), np.float32(0))
    fr.assert_bits(m["depth"], z.astype(np.float32), "depth mean")
    acc.close()


# ------------------------------------------------------------------------------------------------ 4: scheduling independence
@pytest.mark.parametrize("kw", [dict(max_paths=1000), dict(sort_mode=1), dict(sort_mode=6), dict(packet_mode=1), dict(packet_mode=2), dict(global_best=True)],
                         ids=["max_paths_1000", "sort_off", "sort_on", "packet_off", "packet_on", "global_best"])
def test_schedules(textured, kw):
    acc = textured.dev.accumulator(W, H, seed=SEED, features=True)
    st = acc.render(3, **kw)
    if "max_paths" in kw:
        assert st["passes"] > 3  # entries cut over many passes
    acc.render(5, **kw)
    textured.check(acc, str(kw))
    acc.close()


def test_uneven_count_map(textured):
    acc = textured.dev.accumulator(W, H, seed=SEED, features=True)
    acc.render(1)
    thr = float(np.median(_err_at(textured.dev, 2)))
    acc.render_adaptive(thr, min_samples=2, max_samples=N, step=1, max_paths=1024)
    n, _ = textured.check(acc, "adaptive")
    assert len(np.unique(n)) >= 3 and n.min() >= 2 and n.max() == N
    acc.close()


def _err_at(dev, level):
    a = dev.accumulator(W, H, seed=SEED)
    a.render(level)
    a.render_adaptive(0.0, min_samples=2, max_samples=level, step=1)  # a judge that adds nothing
    e = a.read()["error"]
    a.close()
    return e[np.isfinite(e)]


# ------------------------------------------------------------------------------------------------ 5: the wide device build
def test_wide_device_build(gpu, oracle, scenes):
    sc = scenes["boxes"]
    orc = oracle.OracleScene(sc)
    dev = gpu.DeviceScene(sc, device_bvh=True, wide=True)
    rays = fr.primary_rays(orc, W, H, N, SEED)
    op, ob = orc.cast_rays(rays.reshape(-1, 6))
    gp, gb, _ = dev.cast_rays_ex(rays.reshape(-1, 6), gpu.RT_CAST_EXTEND)
    hit_contract.verify_hits(orc, rays.reshape(-1, 6), op, ob, gp, gb, "superset", brute=2000, what="boxes wide primary rays")
    # the contract allows a primary ray whose closest hit the wide tree finds closer (or where the reference's pruning misses): its t replaces the oracle's
    closer = ob[:, 2].view(np.uint32) != gb[:, 2].view(np.uint32)
    print(f"wide tree: {int(closer.sum())} of {len(closer)} primary rays with another t than the oracle's")
    assert closer.sum() < 0.01 * len(closer)
    t = np.where(closer, gb[:, 2], ob[:, 2]).reshape(W * H, N)
    hit = np.where(closer, gp != fr.NONE, op != fr.NONE).reshape(W * H, N)
    assert hit.any() and (~hit).any()
    acc = dev.accumulator(W, H, seed=SEED, features=True)
    acc.render(3, global_best=True)
    acc.render(5, global_best=True)
    f = acc.read_features()
    assert np.array_equal(f["hits"].reshape(-1), fr.hit_ladder(hit)[N])
    fr.assert_bits(f["depth_sum"].reshape(-1), fr.ladder(t)[N], "wide ZS")
    acc.close()
    dev.close()
    orc.close()


# ------------------------------------------------------------------------------------------------ 6: nothing else moved
def test_plain_state_and_counters_unchanged(textured):
    dev = textured.dev
    ref, _ = dev.run_raytracer(W, H, 4, seed=SEED)
    a, b = dev.accumulator(W, H, seed=SEED), dev.accumulator(W, H, seed=SEED, features=True)
    for k in (3, 5):
        sa, sb = a.render(k, counters=True), b.render(k, counters=True)
        for key in COUNTERS:
            assert sa[key] == sb[key], key
        assert sa["passes"] == sb["passes"]
        fb, _ = dev.run_raytracer(W, H, 4, seed=SEED)  # rt_render in between: undisturbed, and disturbs nothing
        assert fr.same_bits(fb, ref)
    sa, sb = a.render_adaptive(0.05, min_samples=4, max_samples=12, step=2, counters=True), b.render_adaptive(0.05, min_samples=4, max_samples=12, step=2, counters=True)
    for key in COUNTERS + ("rounds", "passes"):
        assert sa[key] == sb[key], key
    ra, rb = a.read(), b.read()
    for key in ("sum", "even_sum", "samples", "error"):
        assert fr.same_bits(ra[key], rb[key]), key
    assert fr.same_bits(a.image(), b.image()) and np.array_equal(a.image(rgb8=True), b.image(rgb8=True))
    a.close()
    b.close()


@pytest.mark.parametrize("shape", [(1, 1), (5, 3)])  # (width, height)
def test_small_images(gpu, oracle, scenes, shape):
    w, h = shape
    c = _case(gpu, oracle, scenes, "room_textured", w=w, h=h)
    _split_renders(c, f"{w}x{h}")
    c.dev.close()
    c.orc.close()


# ------------------------------------------------------------------------------------------------ 7: errors
def test_errors(gpu, textured):
    import ctypes as C

    lib, abi = gpu.lib(), gpu._ctypes_abi
    dev = textured.dev
    h = C.c_void_p()
    for flags in (2, 3, 0x80000000):
        assert lib.rt_accum_create_ex(dev._h, W, H, None, 0, flags, C.byref(h)) == 1 and not h.value
    plain_acc = dev.accumulator(W, H, seed=SEED)
    plain_acc.render(2)
    buf = np.zeros((H, W, 3), np.float32)
    assert lib.rt_accum_read_features(plain_acc._h, abi.fptr(buf), None, None, None) == 1
    assert lib.rt_accum_resolve_features(plain_acc._h, 0, buf.ctypes.data_as(C.c_void_p), None, None) == 1
    assert lib.rt_accum_denoise(plain_acc._h, None, 0, buf.ctypes.data_as(C.c_void_p)) == 1
    assert lib.rt_accum_denoise_rgb8(plain_acc._h, None, 0, buf.ctypes.data_as(C.c_void_p)) == 1
    plain_acc.close()
    acc = dev.accumulator(W, H, seed=SEED, features=True)
    acc.render(2)
    assert lib.rt_accum_resolve_features(acc._h, 2, buf.ctypes.data_as(C.c_void_p), None, None) == 1
    for bad in (dict(reserved=(1, 0, 0)), dict(reserved=(0, 0, 7)), dict(iterations=9), dict(sigma_color=-1.0), dict(sigma_depth=-0.5),
                dict(sigma_color=float("nan")), dict(sigma_depth=float("inf")), dict(sigma_color=float("inf")), dict(flags=2), dict(normal_sharpness=9)):
        with pytest.raises(gpu.RtError) as e:
            acc.denoise(**bad)
        assert e.value.code == 1, bad
    assert lib.rt_accum_denoise(acc._h, None, 2, buf.ctypes.data_as(C.c_void_p)) == 1
    assert lib.rt_accum_denoise(acc._h, None, 0, None) == 1
    assert acc.denoise(iterations=8).shape == (H, W, 3)
    acc.close()
