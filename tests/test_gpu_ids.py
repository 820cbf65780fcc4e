"""Id tables of an accumulator with ids (include/rt_abi.h, rt_accum_attach_ids), pinned word for word against the host model
(tests/id_replay.py) fed with the oracle's closest hits of the same primary rays: after every split of the samples over calls, under every
schedule, for every id kind, on the production trees and through a sensor, and without moving anything an accumulator had before. Everything
compared here is an integer or a bit pattern; there is no tolerance. The preconditions of the fixtures are asserted in test_id_replay.py."""
import ctypes as C

import numpy as np
import pytest

import feature_replay as fr
import id_replay as ir
from id_replay import user_table

pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 8
N_TOP = 11  # the adaptive case goes to 8 samples and adds 3 on top
SEED = 7
COUNTERS = ("samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests",
            "light_tri_tests", "light_hits", "texel_fetches")


class _Case:
    """One device scene and the closest hits (`prim`, (pixels, n) as cast_rays reports them) of its accumulators' primary rays."""

    def __init__(self, dev, prim, w=W, h=H):
        self.dev, self.prim, self.w, self.h = dev, prim, w, h
        self._tables = {}

    def tables(self, ids, K):
        key = (ids.tobytes(), K)
        if key not in self._tables:
            self._tables[key] = ir.tables(ids, K)
        return self._tables[key]

    def check(self, acc, ids, K, what):
        """read_ids of `acc` equals the model at every pixel's own n_p; returns (n, the table read)"""
        n = acc.read()["samples"]
        got = acc.read_ids()
        sid, cnt, other = self.tables(ids, K)
        assert got["ids"].shape == got["counts"].shape == (self.h, self.w, K) and got["other"].shape == (self.h, self.w)
        assert np.array_equal(got["counts"], ir.at(cnt, n)), f"{what}: counts"
        assert np.array_equal(got["ids"], ir.at(sid, n)), f"{what}: ids"
        assert np.array_equal(got["other"], ir.at(other, n)), f"{what}: other"
        assert np.array_equal(got["counts"].sum(axis=2) + got["other"], n), f"{what}: counts + other != n"
        return n, got


def _oracle_prims(oracle, scene, n, w=W, h=H):
    orc = oracle.OracleScene(scene)
    _, _, prim = fr.first_hits(orc, fr.primary_rays(orc, w, h, n, SEED))
    orc.close()
    return prim


@pytest.fixture(scope="module")
def plain(gpu, oracle, scenes):
    c = _Case(gpu.DeviceScene(scenes["room_plain"]), _oracle_prims(oracle, scenes["room_plain"], N_TOP))
    yield c
    c.dev.close()


@pytest.fixture(scope="module")
def textured(gpu, oracle, scenes):
    c = _Case(gpu.DeviceScene(scenes["room_textured"]), _oracle_prims(oracle, scenes["room_textured"], N))
    c.sc = scenes["room_textured"]
    yield c
    c.dev.close()


def _split_renders(case, want, K, what, **acc_kw):
    acc = case.dev.accumulator(case.w, case.h, seed=SEED, id_slots=K, **acc_kw)
    total = 0
    for k in (1, 2, 5):  # the calls start at bases 0, 1 and 3
        acc.render(k)
        total += k
        n, got = case.check(acc, want, K, f"{what} after {total}")
        assert np.all(n == total)
    acc.close()
    return got


# ------------------------------------------------------------------------------------------------ 1: split renders, every K
@pytest.mark.parametrize("K", [1, 2, 4, 8, 16])
def test_split_renders_room_plain(plain, K):
    ids = ir.sample_ids(plain.prim[:, :N])
    got = _split_renders(plain, ids, K, f"room_plain K={K}", ids="primitive")
    assert got["other"].any() == (K < 8)  # 1, 2, 4 slots overflow somewhere; 8 and 16 hold every pixel's ids
    assert not got["ids"][got["counts"] == 0].any()  # an empty slot reads id 0


# ------------------------------------------------------------------------------------------------ 2: misses
def test_misses_take_a_slot(gpu, oracle, scenes):
    c = _Case(gpu.DeviceScene(scenes["open_nolight"]), _oracle_prims(oracle, scenes["open_nolight"], N))
    got = _split_renders(c, ir.sample_ids(c.prim), 2, "open_nolight", ids="primitive")
    miss = (got["ids"] == ir.MISS) & (got["counts"] > 0)
    real = (got["ids"] != ir.MISS) & (got["counts"] > 0)
    assert (miss.any(axis=2) & real.any(axis=2)).any() and got["other"].any()
    c.dev.close()


# ------------------------------------------------------------------------------------------------ 3: material and user ids
def test_material_ids(textured):
    _split_renders(textured, ir.sample_ids(textured.prim, "material", material_ids=textured.sc.material_ids), 4, "room_textured material", ids="material")


def test_user_ids_from_a_host_and_a_device_table(textured):
    import torch

    tab = user_table(len(textured.sc.material_ids))
    ids = ir.sample_ids(textured.prim, "user", table=tab)
    dtab = torch.from_numpy(tab.view(np.int32)).to(f"cuda:{textured.dev._device}")
    torch.cuda.synchronize()
    a = textured.dev.accumulator(W, H, seed=SEED, ids=tab, id_slots=4)
    b = textured.dev.accumulator(W, H, seed=SEED)
    b.attach_ids(dtab.data_ptr(), slots=4, n_table=len(tab))
    tab[:] = 0  # the table was copied at attach
    dtab.zero_()
    torch.cuda.synchronize()
    for k in (3, 5):
        a.render(k)
        b.render(k)
    _, ga = textured.check(a, ids, 4, "user ids, host table")
    _, gb = textured.check(b, ids, 4, "user ids, device table")
    for key in ga:
        assert np.array_equal(ga[key], gb[key]), key
    assert ((ga["ids"] == ir.MISS) & (ga["counts"] > 0)).any()
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4: analytic primitives
def test_analytic_primitives(gpu, oracle):
    from conftest import SCENE000

    ls = gpu.parse_scene_txt(SCENE000)
    a = ls.arrays()
    c = _Case(gpu.DeviceScene(ls), _oracle_prims(oracle, ls, N))
    assert (c.prim == 12).any() and (c.prim == 13).any()  # the ELLIPSOID and the PLANE win primary rays
    got = _split_renders(c, ir.sample_ids(c.prim), 4, "scene-000.txt primitive", ids="primitive")
    held = got["ids"][got["counts"] > 0]
    assert (held == 12).any() and (held == 13).any()
    pm = [p["material_id"] for p in a["primitives"]]
    mat = ir.sample_ids(c.prim, "material", material_ids=a["material_ids"], prim_materials=pm)
    _split_renders(c, mat, 4, "scene-000.txt material", ids="material")
    c.dev.close()


# ------------------------------------------------------------------------------------------------ 5: schedules
@pytest.mark.parametrize("kw", [dict(max_paths=1024), dict(sort_mode=1), dict(sort_mode=6), dict(packet_mode=1), dict(packet_mode=2)],
                         ids=["max_paths_1024", "sort_off", "sort_on", "packet_off", "packet_on"])
def test_schedules(plain, kw):
    ids = ir.sample_ids(plain.prim)
    acc = plain.dev.accumulator(W, H, seed=SEED, ids="primitive", id_slots=2)
    st = acc.render(N, **kw)
    if "max_paths" in kw:
        assert st["passes"] == W * H * N // 1024  # 24 passes of the 24 576 paths
    n, got = plain.check(acc, ids, 2, str(kw))
    assert np.all(n == N) and got["other"].any()
    acc.close()


def test_adaptive_counts_and_a_render_on_top(plain):
    ids = ir.sample_ids(plain.prim)
    probe = plain.dev.accumulator(W, H, seed=SEED)
    probe.render(2)
    probe.render_adaptive(0.0, min_samples=2, max_samples=2, step=1)  # a judge that adds nothing
    err = probe.read()["error"]
    probe.close()
    thr = float(np.median(err[np.isfinite(err)]))
    for K in (2, 4):
        acc = plain.dev.accumulator(W, H, seed=SEED, ids="primitive", id_slots=K)
        acc.render_adaptive(thr, min_samples=2, max_samples=N, step=3, max_paths=1024)
        n, _ = plain.check(acc, ids, K, f"adaptive K={K}")
        assert len(np.unique(n)) >= 2 and n.min() >= 2 and n.max() == N  # n_p varies
        acc.render(3)
        n2, _ = plain.check(acc, ids, K, f"adaptive + 3, K={K}")
        assert np.array_equal(n2, n + 3)
        acc.close()


# ------------------------------------------------------------------------------------------------ 6: the production trees
def test_production_trees(gpu, oracle, scenes):
    sc = scenes["room_plain"]
    orc = oracle.OracleScene(sc)
    dev = gpu.DeviceScene(sc, wide=True, device_bvh=True)
    sn = gpu.Sensor.pinhole(sc.camera, seed=SEED)
    rays = dev.sensor_rays(sn, W, H, N)
    od = np.concatenate([rays["origin"], rays["dir"]], axis=1).astype(np.float32)
    gp, gb, _ = dev.cast_rays_ex(od, gpu.RT_CAST_EXTEND)
    op, ob = orc.cast_rays(od)
    differ = gp != op
    print(f"wide device tree: {int(differ.sum())} of {len(gp)} primary rays report another prim than the oracle")
    # the production hit contract: another index only for an exact tie
    assert np.array_equal(gb[differ, 2].view(np.uint32), ob[differ, 2].view(np.uint32))
    assert not ((gp == ir.MISS) ^ (op == ir.MISS))[differ].any()
    c = _Case(dev, gp.reshape(W * H, N))
    ids = ir.sample_ids(c.prim)
    for K in (2, 8):
        acc = dev.accumulator(W, H, sensor=sn, ids="primitive", id_slots=K)
        acc.render(3, global_best=True)
        acc.render(5, global_best=True)
        n, _ = c.check(acc, ids, K, f"wide device tree, global best, K={K}")
        assert np.all(n == N)
        acc.close()
    dev.close()
    orc.close()


# ------------------------------------------------------------------------------------------------ 7: a sensor accumulator
def test_equirect_sensor(gpu, oracle, textured):
    sn = gpu.Sensor.equirect(textured.sc.camera, seed=SEED)
    rays = textured.dev.sensor_rays(sn, W, H, N)
    od = np.concatenate([rays["origin"], rays["dir"]], axis=1).astype(np.float32)
    orc = oracle.OracleScene(textured.sc)
    prim, _ = orc.cast_rays(od)
    orc.close()
    c = _Case(textured.dev, prim.reshape(W * H, N))
    ids = ir.sample_ids(c.prim)
    assert not np.array_equal(c.prim, textured.prim) and ir.distinct_per_pixel(ids).max() >= 2  # another view than the pinhole's, with mixed pixels
    acc = textured.dev.accumulator(W, H, sensor=sn, ids="primitive", id_slots=4)
    for k in (3, 5):
        acc.render(k)
        c.check(acc, ids, 4, "equirect")
    acc.close()


# ------------------------------------------------------------------------------------------------ 8: nothing else moves
def test_everything_else_is_unchanged(textured):
    dev = textured.dev
    a = dev.accumulator(W, H, seed=SEED, features=True)
    b = dev.accumulator(W, H, seed=SEED, features=True, ids="material", id_slots=2)
    for k in (3, 2):
        sa, sb = a.render(k, counters=True), b.render(k, counters=True)
        for key in COUNTERS + ("passes",):
            assert sa[key] == sb[key], key
    ad = dict(min_samples=6, max_samples=12, step=2, counters=True)
    sa, sb = a.render_adaptive(0.05, **ad), b.render_adaptive(0.05, **ad)
    for key in COUNTERS + ("rounds", "passes"):
        assert sa[key] == sb[key], key
    ra, rb = a.read(), b.read()
    for key in ("sum", "even_sum", "samples", "error"):
        assert fr.same_bits(ra[key], rb[key]), key
    fa, fb = a.read_features(), b.read_features()
    for key in ("albedo_sum", "normal_sum", "depth_sum", "hits"):
        assert fr.same_bits(fa[key], fb[key]), key
    assert fr.same_bits(a.image(), b.image()) and np.array_equal(a.image(rgb8=True), b.image(rgb8=True))
    t = b.read_ids()
    assert np.array_equal(t["counts"].sum(axis=2) + t["other"], rb["samples"])
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 9: labels and matte
def test_labels_and_matte(textured):
    import torch

    dev = textured.dev
    tab = user_table(len(textured.sc.material_ids))
    ids = ir.sample_ids(textured.prim, "user", table=tab)
    id_set = [1, 3, 1, 77, ir.MISS]  # a duplicate, an absent id, RT_ID_MISS
    assert (ids == 1).any() and (ids == 3).any() and (ids == ir.MISS).any() and not (ids == 77).any()
    for K in (2, 4):
        sid, cnt, _ = textured.tables(ids, K)
        acc = dev.accumulator(W, H, seed=SEED, ids=tab, id_slots=K)
        d_label = torch.full((H, W), 5, dtype=torch.int32, device=f"cuda:{dev._device}")
        d_cov = torch.full((H, W), 5.0, dtype=torch.float32, device=f"cuda:{dev._device}")
        d_matte = torch.full((H, W), 5.0, dtype=torch.float32, device=f"cuda:{dev._device}")
        torch.cuda.synchronize()
        for total, k in ((0, 0), (2, 2), (8, 6)):  # n_p = 0 before the first render; level 2 holds 1 : 1 ties
            if k:
                acc.render(k)
            n = np.full((H, W), total, np.uint32)
            want_label, want_cov = ir.labels(ir.at(sid, n), ir.at(cnt, n), n)
            want_matte = ir.matte(ir.at(sid, n), ir.at(cnt, n), n, id_set)
            label, cov = acc.labels()
            assert label.dtype == np.uint32 and np.array_equal(label, want_label), (K, total)
            fr.assert_bits(cov, want_cov, f"coverage K={K} n={total}")
            fr.assert_bits(acc.matte(id_set), want_matte, f"matte K={K} n={total}")
            assert acc.labels(device_out=(d_label.data_ptr(), d_cov.data_ptr())) == (None, None)
            assert acc.matte(id_set, device_out=d_matte.data_ptr()) is None
            assert np.array_equal(d_label.cpu().numpy().view(np.uint32), want_label)
            fr.assert_bits(d_cov.cpu().numpy(), want_cov, "device coverage")
            fr.assert_bits(d_matte.cpu().numpy(), want_matte, "device matte")
            if total == 0:
                assert np.all(label == ir.MISS) and not cov.any() and not want_matte.any()
            if total == 2:
                tie = ir.at(cnt, n)[..., 1] == 1  # two ids, one sample each: the label is the first seen
                assert tie.any() and np.array_equal(label[tie], ids.reshape(H, W, N)[..., 0][tie])
        # either output alone
        only_cov = torch.zeros((H, W), dtype=torch.float32, device=f"cuda:{dev._device}")
        torch.cuda.synchronize()
        acc.labels(device_out=(None, only_cov.data_ptr()))
        fr.assert_bits(only_cov.cpu().numpy(), want_cov, "coverage alone")
        assert 0 < np.count_nonzero(want_matte) and (want_matte < 1).any()
        acc.close()


# ------------------------------------------------------------------------------------------------ 10: errors
def test_errors(gpu, oracle, scenes):
    import torch

    lib, abi = gpu.lib(), gpu._ctypes_abi
    w, h, n_max = 16, 12, 20
    sc = scenes["room_textured"]
    dev = gpu.DeviceScene(sc)
    c = _Case(dev, _oracle_prims(oracle, sc, n_max, w=w, h=h), w=w, h=h)
    ids = ir.sample_ids(c.prim)
    n_tab = len(sc.material_ids)
    tab = user_table(n_tab)
    dtab = torch.from_numpy(tab.view(np.int32)).to(f"cuda:{dev._device}")
    torch.cuda.synchronize()

    def desc(kind=abi.RT_ID_PRIMITIVE, slots=4, table=None, n_table=0, flags=0, reserved=(0, 0)):
        d = abi.RtIdDesc(kind, slots, table, n_table, flags)
        d.reserved[0], d.reserved[1] = reserved
        return d

    bad = {
        "unknown kind": desc(kind=3),
        "unknown kind, high bit": desc(kind=0x80000000),
        "17 slots": desc(slots=17),
        "reserved[0]": desc(reserved=(1, 0)),
        "reserved[1]": desc(reserved=(0, 9)),
        "unknown flag": desc(flags=2),
        "unknown flag beside DEVICE_FB": desc(kind=abi.RT_ID_USER, table=dtab.data_ptr(), n_table=n_tab, flags=abi.RT_FLAG_DEVICE_FB | 8),
        "user without a table": desc(kind=abi.RT_ID_USER, n_table=n_tab),
        "user table too short": desc(kind=abi.RT_ID_USER, table=tab.ctypes.data, n_table=n_tab - 1),
        "user table too long": desc(kind=abi.RT_ID_USER, table=tab.ctypes.data, n_table=n_tab + 1),
        "primitive with a table": desc(table=tab.ctypes.data),
        "material with n_table": desc(kind=abi.RT_ID_MATERIAL, n_table=n_tab),
        "misaligned device table": desc(kind=abi.RT_ID_USER, table=dtab.data_ptr() + 2, n_table=n_tab, flags=abi.RT_FLAG_DEVICE_FB),
    }
    assert lib.rt_accum_attach_ids(None, C.byref(desc())) == 1

    # an accumulator with ids: every refusal (a second attach among them) leaves it as it was: one more sample, and the table is the model's
    acc = dev.accumulator(w, h, seed=SEED, ids="primitive", id_slots=4)
    bad_again = dict(bad, **{"a second attach": desc(), "a second attach, other kind": desc(kind=abi.RT_ID_MATERIAL, slots=2)})
    assert len(bad_again) + 1 <= n_max
    for what, d in bad_again.items():
        assert lib.rt_accum_attach_ids(acc._h, C.byref(d)) == 1, what
        assert b"rt_accum_attach_ids" in lib.rt_last_error(), what
        acc.render(1)
        c.check(acc, ids, 4, f"after the refusal of {what}")
    assert lib.rt_accum_attach_ids(acc._h, None) == 1
    # the reads
    u32 = np.zeros(w * h, np.uint32)
    f32 = np.zeros(w * h, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.rt_accum_resolve_labels(acc._h, 2, vp(u32), vp(f32)) == 1
    assert lib.rt_accum_resolve_matte(acc._h, 2, abi.u32ptr(u32), 4, vp(f32)) == 1
    assert lib.rt_accum_resolve_matte(acc._h, 0, None, 4, vp(f32)) == 1
    assert lib.rt_accum_resolve_matte(acc._h, 0, abi.u32ptr(u32), 4, None) == 1
    big = np.zeros(4097, np.uint32)
    assert lib.rt_accum_resolve_matte(acc._h, 0, abi.u32ptr(big), 0, vp(f32)) == 1
    assert lib.rt_accum_resolve_matte(acc._h, 0, abi.u32ptr(big), 4097, vp(f32)) == 1
    assert lib.rt_accum_resolve_matte(acc._h, 0, abi.u32ptr(big), 4096, vp(f32)) == 0
    acc.render(1)
    c.check(acc, ids, 4, "after the refused reads")
    acc.close()

    # a fresh accumulator: the same refusals, then a valid attach still works and the table is the model's
    fresh = dev.accumulator(w, h, seed=SEED)
    for what, d in bad.items():
        assert lib.rt_accum_attach_ids(fresh._h, C.byref(d)) == 1, what
        assert lib.rt_accum_read_ids(fresh._h, abi.u32ptr(u32), None, None) == 1, what
    fresh.attach_ids("primitive", slots=2)
    fresh.render(3)
    c.check(fresh, ids, 2, "fresh accumulator after the refusals")
    fresh.close()

    # an accumulator that holds samples takes no ids, and one without ids refuses the three reads, before and after
    late = dev.accumulator(w, h, seed=SEED)

    def reads_refused():
        assert lib.rt_accum_read_ids(late._h, abi.u32ptr(u32), abi.u32ptr(u32), abi.u32ptr(u32)) == 1
        assert lib.rt_accum_resolve_labels(late._h, 0, vp(u32), vp(f32)) == 1
        assert lib.rt_accum_resolve_matte(late._h, 0, abi.u32ptr(u32), 4, vp(f32)) == 1

    reads_refused()
    late.render(1)
    assert lib.rt_accum_attach_ids(late._h, C.byref(desc())) == 1
    with pytest.raises(gpu.RtError) as e:
        late.attach_ids("material")
    assert e.value.code == 1
    reads_refused()
    late.render(1)
    assert np.all(late.read()["samples"] == 2)
    late.close()
    dev.close()
