"""Light groups of an accumulator (include/rt_abi.h, rt_accum_attach_light_groups) on the device. The exact check (tests/light_groups.py): in
a scene whose groups emit in one colour channel each, group g's sum is channel g of the ungrouped sum S, bit for bit, and zero elsewhere; S is
the oracle's samples added in sample order on the parity tree, and the accumulator's own S on the production traversals (global-best pruning
and the wide tree return other hits than the oracle on ties and on the hits its near-local pruning skips: the production hit contract). Then
every schedule, general colours against the oracle's images of one group at a time, the other emitters and cameras, the resolves, the refusals
and the CLI; and nothing an accumulator had before moves. The preconditions of the fixtures are asserted in test_light_group_fixtures.py."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import light_groups as lg
from light_groups import COUNTERS, H, N, NONE, SEED, W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = min(16, int(os.environ.get("OMP_NUM_THREADS") or 16))


class _Case:
    """A channel-separated scene on the parity tree: the device scene, its groups and the oracle's S of N samples per pixel."""

    def __init__(self, gpu, oracle, scene, ray_depth=None):
        self.sc, self.mg, self.bg = lg.channel_scene(scene)
        if ray_depth is not None:
            self.sc.ray_depth = ray_depth
        orc = oracle.OracleScene(self.sc)
        self.x = orc.pixel_samples(W, H, N, np.arange(W * H), seed=SEED, threads=THREADS).reshape(H, W, N, 3)
        orc.close()
        self.S = lg.fold_sum(self.x)
        self.dev = gpu.DeviceScene(self.sc)
        self._ref = None

    def groups(self, **kw):
        return dict(dict(material_group=self.mg, background=self.bg), **kw)

    def accumulator(self, dev=None, **kw):
        return (dev or self.dev).accumulator(W, H, seed=SEED, light_groups=self.groups(), **kw)

    def reference(self):
        """GS of one render of N samples, default schedule: computed once, compared against, never modified."""
        if self._ref is None:
            acc = self.accumulator()
            acc.render(N)
            self._ref = acc.read_light_groups()
            self._ref.setflags(write=False)
            acc.close()
        return self._ref


@pytest.fixture(scope="module")
def room(gpu, oracle, scenes):
    c = _Case(gpu, oracle, scenes["room_plain"])
    yield c
    c.dev.close()


@pytest.fixture(scope="module")
def boxes(gpu, oracle, scenes):
    c = _Case(gpu, oracle, scenes["boxes"])
    yield c
    c.dev.close()


def _own(acc, what):
    """The exact check of an accumulator against its own S; returns (GS, state)."""
    r = acc.read()
    GS = acc.read_light_groups()
    lg.assert_channels(GS, r["sum"], what=what)
    return GS, r


# ------------------------------------------------------------------------------------------------ 1: the exact check
@pytest.mark.parametrize("name", ["room", "boxes"])
def test_exact_on_the_parity_tree(request, name):
    c = request.getfixturevalue(name)
    GS = c.reference()
    assert GS.shape == (3, H, W, 3)
    lg.assert_channels(GS, c.S, what=f"{name} against the oracle")
    for k in range(3):
        print(f"{name}: group {k} holds channel {k} above zero in {(GS[k, ..., k] > 0).mean():.3f} of the pixels")
        assert (GS[k, ..., k] > 0).any()


@pytest.mark.parametrize("name", ["room", "boxes"])
def test_exact_with_global_best(request, name):
    c = request.getfixturevalue(name)
    acc = c.accumulator()
    acc.render(N, global_best=True)
    GS, r = _own(acc, f"{name}, global best")
    assert np.all(r["samples"] == N) and all((GS[k, ..., k] > 0).any() for k in range(3))
    acc.close()


@pytest.mark.parametrize("name", ["room", "boxes"])
def test_exact_on_the_wide_device_tree(gpu, request, name):
    c = request.getfixturevalue(name)
    dev = gpu.DeviceScene(c.sc, wide=True, device_bvh=True)
    for gb in (False, True):
        acc = c.accumulator(dev)
        acc.render(3, global_best=gb)
        acc.render(5, global_best=gb)
        GS, r = _own(acc, f"{name}, wide device tree, global_best={gb}")
        assert np.all(r["samples"] == N) and all((GS[k, ..., k] > 0).any() for k in range(3))
        acc.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ 2: schedules
def _same_as_reference(c, acc, what):
    GS = acc.read_light_groups()
    lg.assert_channels(GS, c.S, what=what)
    assert lg.same_bits(GS, c.reference()), f"{what}: not the sums of one render of {N}"


def test_split_renders(room):
    acc = room.accumulator()
    total = 0
    for k in (1, 2, 5):  # the calls start at bases 0, 1 and 3
        acc.render(k)
        total += k
        lg.assert_channels(acc.read_light_groups(), lg.fold_sum(room.x[:, :, :total]), what=f"after {total}")
    _same_as_reference(room, acc, "split 1, 2, 5")
    acc.close()


@pytest.mark.parametrize("kw", [dict(max_paths=1000), dict(max_paths=4096), dict(), dict(sort_mode=1), dict(sort_mode=6), dict(packet_mode=1), dict(packet_mode=2),
                                dict(max_paths=1000, sort_mode=6, packet_mode=2)],
                         ids=["max_paths_1000", "max_paths_4096", "default", "sort_off", "sort_on", "packet_off", "packet_on", "small_sorted_packets"])
def test_schedules(room, kw):
    acc = room.accumulator()
    st = acc.render(N, **kw)
    if kw.get("max_paths") == 1000:
        assert st["passes"] == W * H * N // 1024  # the library's floor of max_paths is 1024: 24 passes, and many passes leave stale tags behind
    _same_as_reference(room, acc, str(kw))
    acc.close()


@pytest.mark.parametrize("depth", [1, 2, 8])
@pytest.mark.parametrize("name", ["room_plain", "boxes"])
def test_ray_depths(gpu, oracle, scenes, name, depth):
    """Depths 1 and 2 cut almost every path at depth_left == 0 straight after a push: the terminal level's tag is stale there. At depth 1 a
    sample is the background of a primary miss or the emission of the primary hit: the closed room is then black but for lights in view."""
    c = _Case(gpu, oracle, scenes[name], ray_depth=depth)
    for kw in (dict(), dict(max_paths=1000)):
        acc = c.accumulator()
        acc.render(3, **kw)
        acc.render(5, **kw)
        lg.assert_channels(acc.read_light_groups(), c.S, what=f"ray_depth {depth} {kw}")
        acc.close()
    lit = [bool((c.S[..., k] > 0).any()) for k in range(3)]
    print(f"{name} at ray_depth {depth}: channels above zero somewhere: {lit}")
    assert (lit[0] and lit[1]) or depth == 1
    assert lit[2] or name == "room_plain"
    c.dev.close()


def _median_err(dev, samples=2, **acc_kw):
    """A threshold that splits the pixels: the median finite err after `samples` samples, read from a judge that adds nothing."""
    probe = dev.accumulator(W, H, seed=SEED, **acc_kw)
    probe.render(samples)
    probe.render_adaptive(0.0, min_samples=samples, max_samples=samples, step=1)
    err = probe.read()["error"]
    probe.close()
    return float(np.median(err[np.isfinite(err)]))


def test_adaptive_at_every_pixels_own_count(room):
    for thr, varied in ((0.05, False), (_median_err(room.dev), True)):  # the second threshold stops some pixels early: n_p varies
        acc = room.accumulator()
        acc.render_adaptive(thr, min_samples=2, max_samples=11, step=3)
        GS, r = _own(acc, f"adaptive, threshold {thr}")
        n = r["samples"]
        print(f"adaptive, threshold {thr}: counts", np.unique(n))
        assert n.min() >= 2 and n.max() <= 11 and (len(np.unique(n)) >= 2 or not varied)
        m = n <= N  # where the oracle's samples reach: against the oracle too
        want = lg.fold_sum(room.x, counts=np.minimum(n, N))
        for k in range(3):
            assert lg.same_bits(GS[k, ..., k][m], want[..., k][m]), k
        assert m.any() or not varied
        acc.close()


# ------------------------------------------------------------------------------------------------ 3: general colours, five groups
def test_five_groups_with_ordinary_colours(gpu, oracle, scenes):
    sc, mg, bg, G = lg.five_group_scene(scenes["room_plain"])
    dev = gpu.DeviceScene(sc)
    acc = dev.accumulator(W, H, seed=SEED, light_groups=dict(material_group=mg, background=bg, n_groups=G))
    acc.render(N)
    full = acc.image()
    orc = oracle.OracleScene(sc)
    ref_full, ref_st = orc.run_raytracer(W, H, N, seed=SEED)
    orc.close()
    assert lg.same_bits(full, ref_full)
    GS = acc.read_light_groups()
    assert GS.shape == (G, H, W, 3) and np.all(GS[3] == 0)  # the empty group is exactly 0
    total = np.zeros_like(full)
    for g in (0, 1, 2, 4):
        one = lg.only_group(sc, mg, bg, g)
        o = oracle.OracleScene(one)
        ref, st = o.run_raytracer(W, H, N, seed=SEED)
        o.close()
        for key in COUNTERS:
            assert st[key] == ref_st[key], (g, key)  # the scaled scene has the same light tree and the same paths
        img = acc.light_group(g)
        err = np.abs(img.astype(np.float64) - ref.astype(np.float64))
        bound = 2.0 ** -90 * (1.0 + ref_full.astype(np.float64))
        print(f"group {g}: max |group image - oracle image of the group alone| = {err.max():.3e}, max of the image {img.max():.3e}")
        assert np.all(err <= bound), g
        assert (img > 0).any()
        total += img
    # the groups add up to the image as far as float addition allows (the header promises no more)
    assert np.allclose(total, full, rtol=1e-5, atol=1e-6)
    acc.close()
    dev.close()


def test_a_material_in_no_group(room):
    """RT_LIGHT_GROUP_NONE: the green lights are in S and in no group."""
    mg = [None if g == 1 else g for g in room.mg]
    acc = room.dev.accumulator(W, H, seed=SEED, light_groups=dict(material_group=mg, background=room.bg, n_groups=3))
    acc.render(N)
    GS = acc.read_light_groups()
    lg.assert_channels(GS, room.S, groups=(0, None, 2), what="green in no group")
    assert np.all(GS[1] == 0) and (room.S[..., 1] > 0).any()
    # ... and a background in no group
    acc2 = room.dev.accumulator(W, H, seed=SEED, light_groups=dict(material_group=room.mg, background=None, n_groups=2))
    acc2.render(N)
    GS2 = acc2.read_light_groups()
    assert GS2.shape[0] == 2
    lg.assert_channels(GS2, room.S, groups=(0, 1), what="background in no group")
    assert lg.same_bits(acc2.read()["sum"], room.S)
    acc.close()
    acc2.close()


# ------------------------------------------------------------------------------------------------ 4: other emitters, backgrounds, cameras
@pytest.mark.parametrize("importance", [False, True], ids=["plain", "importance"])
def test_float_environment(gpu, boxes, importance):
    rng = np.random.default_rng(5)
    env = np.zeros((16, 32, 3), dtype=np.float32)
    env[..., 2] = rng.uniform(0.1, 3.0, size=(16, 32)).astype(np.float32)
    env[3, 7, 2] = 40.0  # a sun
    dev = gpu.DeviceScene(boxes.sc)
    dev.set_environment(env, importance=importance)
    acc = boxes.accumulator(dev)
    acc.render(3)
    acc.render(5)
    GS, r = _own(acc, f"float environment, importance={importance}")
    assert (GS[2, ..., 2] > 0).mean() > 0.9 and (GS[0, ..., 0] > 0).any() and (GS[1, ..., 1] > 0).any()
    assert not lg.same_bits(r["sum"], boxes.S)  # the environment is what lights the misses
    acc.close()
    dev.close()


def test_emissive_ellipsoid(gpu, sg):
    from conftest import SCENE000

    a = gpu.parse_scene_txt(SCENE000).arrays()
    sc = sg.scene_from_arrays(a)
    ell = [i for i, p in enumerate(sc.primitives) if int(p["kind"]) == 1]  # RT_PRIM_ELLIPSOID
    assert ell
    for m in sc.materials:  # nobody else emits green
        m.emission = (m.emission[0], 0.0, m.emission[2])
    sc.bg_color = (sc.bg_color[0], 0.0, sc.bg_color[2])
    glow = copy.deepcopy(sc.materials[sc.primitives[ell[0]]["material_id"]])
    glow.emission = (0.0, 0.9, 0.0)
    sc.materials.append(glow)
    sc.primitives = [dict(p) for p in sc.primitives]
    sc.primitives[ell[0]]["material_id"] = len(sc.materials) - 1
    mg = [None] * len(sc.materials)
    mg[-1] = 0
    dev = gpu.DeviceScene(sc)
    acc = dev.accumulator(W, H, seed=SEED, light_groups=dict(material_group=mg, n_groups=1))
    acc.render(3)
    acc.render(5)
    S = acc.read()["sum"]
    GS = acc.read_light_groups()
    lg.assert_channels(GS, S, groups=(None, 0, None), what="ellipsoid")
    print(f"ellipsoid: its group is above zero in {(GS[0, ..., 1] > 0).mean():.3f} of the pixels")
    assert (GS[0, ..., 1] > 0).any()
    acc.close()
    dev.close()


def test_fisheye_sensor(gpu, room):
    sn = gpu.Sensor.fisheye(room.sc.camera, seed=SEED)
    acc = room.dev.accumulator(W, H, sensor=sn, light_groups=room.groups())
    acc.render(3)
    acc.render(5)
    GS, r = _own(acc, "fisheye")
    assert not lg.same_bits(r["sum"], room.S) and (GS[0, ..., 0] > 0).mean() > 0.5
    acc.close()


# ------------------------------------------------------------------------------------------------ 5: nothing else moves
def test_everything_else_is_unchanged(gpu, scenes):
    sc, mg, bg, G = lg.five_group_scene(scenes["room_textured"])
    dev = gpu.DeviceScene(sc)
    a = dev.accumulator(W, H, seed=SEED, features=True, ids="material", id_slots=2)
    b = dev.accumulator(W, H, seed=SEED, features=True, ids="material", id_slots=2, light_groups=dict(material_group=mg, background=bg, n_groups=G))
    for k in (3, 2):
        sa, sb = a.render(k, counters=True), b.render(k, counters=True)
        for key in COUNTERS + ("passes",):
            assert sa[key] == sb[key], key
    ad = dict(min_samples=6, max_samples=12, step=2, counters=True)
    thr = _median_err(dev, samples=6)
    sa, sb = a.render_adaptive(thr, **ad), b.render_adaptive(thr, **ad)
    for key in COUNTERS + ("rounds", "passes"):
        assert sa[key] == sb[key], key
    ra, rb = a.read(), b.read()
    assert len(np.unique(ra["samples"])) >= 2
    assert np.array_equal(ra["samples"], rb["samples"])
    for key in ("sum", "even_sum", "error"):
        assert lg.same_bits(ra[key], rb[key]), key
    fa, fb = a.read_features(), b.read_features()
    for key in ("albedo_sum", "normal_sum", "depth_sum"):
        assert lg.same_bits(fa[key], fb[key]), key
    assert np.array_equal(fa["hits"], fb["hits"])
    ia, ib = a.read_ids(), b.read_ids()
    for key in ("ids", "counts", "other"):
        assert np.array_equal(ia[key], ib[key]), key
    assert lg.same_bits(a.image(), b.image()) and np.array_equal(a.image(rgb8=True), b.image(rgb8=True))
    assert lg.same_bits(a.denoise(), b.denoise())
    GS = b.read_light_groups()
    assert (GS[0] > 0).any() and np.all(GS[3] == 0) and np.allclose(GS.sum(axis=0), rb["sum"], rtol=1e-4, atol=1e-5)
    a.close()
    b.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ 6: the resolves
def test_resolves(gpu, scenes):
    import torch

    sc, mg, bg, G = lg.five_group_scene(scenes["boxes"])
    dev = gpu.DeviceScene(sc)
    dmg = torch.from_numpy(np.array([NONE if g is None else g for g in mg], dtype=np.uint32).view(np.int32)).to(f"cuda:{dev._device}")
    torch.cuda.synchronize()
    acc = dev.accumulator(W, H, seed=SEED, light_groups=dict(material_group=mg, background=bg, n_groups=G))
    dacc = dev.accumulator(W, H, seed=SEED)
    dacc.attach_light_groups(dmg.data_ptr(), background=bg, n_groups=G, n_materials=len(mg))
    dmg.zero_()  # the table was copied at attach
    torch.cuda.synchronize()
    rng = np.random.default_rng(17)
    weights = {"random": rng.uniform(-0.5, 2.0, size=(G, 3)).astype(np.float32), "ones": np.ones((G, 3), np.float32)}
    for g in range(G):
        weights[f"one-hot {g}"] = np.eye(G, dtype=np.float32)[g][:, None].repeat(3, axis=1)
    d_out = torch.full((H, W, 3), 5.0, dtype=torch.float32, device=f"cuda:{dev._device}")
    d_rgb8 = torch.full((H, W, 3), 5, dtype=torch.uint8, device=f"cuda:{dev._device}")
    torch.cuda.synchronize()
    for total, k in ((0, 0), (3, 3), (8, 5)):  # n_p = 0 before the first render
        if k:
            acc.render(k)
            dacc.render(k)
        n = acc.read()["samples"]
        assert np.all(n == total)
        GS = acc.read_light_groups()
        assert lg.same_bits(GS, dacc.read_light_groups()), "device material table"
        for g in range(G):
            want = lg.group_mean(GS[g], n)
            assert lg.same_bits(acc.light_group(g), want), (total, g)
            assert acc.light_group(g, device_out=d_out.data_ptr()) is None
            assert lg.same_bits(d_out.cpu().numpy(), want), (total, g, "device")
        for name, w in weights.items():
            want = lg.mix_model(GS, n, w)
            got = acc.light_mix(w)
            assert lg.same_bits(got, want), (total, name)
            assert np.array_equal(acc.light_mix(w, rgb8=True), gpu.tonemap(got)), (total, name, "rgb8")
            assert acc.light_mix(w, device_out=d_out.data_ptr()) is None
            assert lg.same_bits(d_out.cpu().numpy(), want), (total, name, "device")
            assert acc.light_mix(w, rgb8=True, device_out=d_rgb8.data_ptr()) is None
            assert np.array_equal(d_rgb8.cpu().numpy(), gpu.tonemap(got)), (total, name, "device rgb8")
            if name.startswith("one-hot") and total:
                assert np.array_equal(got == 0, lg.group_mean(GS[int(name.split()[1])], n) == 0)
        if total == 0:
            assert not acc.light_mix(weights["random"]).any()
    one = acc.light_mix(np.ones(G, np.float32))  # (G,) weights: one factor per group
    assert lg.same_bits(one, acc.light_mix(weights["ones"])) and np.allclose(one, acc.image(), rtol=1e-5, atol=1e-6)
    acc.close()
    dacc.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_errors(gpu, scenes):
    import torch

    lib, abi = gpu.lib(), gpu._ctypes_abi
    w, h = 16, 12
    sc, mg, bg = lg.channel_scene(scenes["room_plain"])
    dev = gpu.DeviceScene(sc)
    n_mat = len(mg)
    tab = np.array([NONE if g is None else g for g in mg], dtype=np.uint32)
    dtab = torch.from_numpy(tab.view(np.int32)).to(f"cuda:{dev._device}")
    torch.cuda.synchronize()
    plain = dev.accumulator(w, h, seed=SEED)
    ladder = [plain.read()["sum"]]

    def plain_at(level):
        while len(ladder) <= level:
            plain.render(1)
            ladder.append(plain.read()["sum"])
        return ladder[level]

    def desc(n_groups=3, background=bg, table=tab.ctypes.data, n_materials=n_mat, flags=0, reserved=(0, 0)):
        d = abi.RtLightGroupDesc(n_groups, background, table, n_materials, flags)
        d.reserved[0], d.reserved[1] = reserved
        return d

    high = tab.copy()
    high[1] = 3
    bad = {
        "no groups": desc(n_groups=0),
        "nine groups": desc(n_groups=9),
        "a material entry == G": desc(table=high.ctypes.data),
        "a material entry >= G with fewer groups": desc(n_groups=1, background=0),
        "background == G": desc(background=3),
        "background far above": desc(background=0x80000000),
        "one material too few": desc(n_materials=n_mat - 1),
        "one material too many": desc(n_materials=n_mat + 1),
        "no table": desc(table=None),
        "reserved[0]": desc(reserved=(1, 0)),
        "reserved[1]": desc(reserved=(0, 9)),
        "unknown flag": desc(flags=2),
        "unknown flag beside DEVICE_FB": desc(table=dtab.data_ptr(), flags=abi.RT_FLAG_DEVICE_FB | 8),
        "misaligned device table": desc(table=dtab.data_ptr() + 2, flags=abi.RT_FLAG_DEVICE_FB),
    }
    assert lib.rt_accum_attach_light_groups(None, C.byref(desc())) == 1

    f32 = np.zeros(3 * w * h * 3, np.float32)
    u8 = np.zeros(w * h * 3, np.uint8)
    wts = np.ones((3, 3), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def check(acc, level, what):
        r = acc.read()
        assert np.all(r["samples"] == level) and lg.same_bits(r["sum"], plain_at(level)), what
        lg.assert_channels(acc.read_light_groups(), r["sum"], what=what)

    # an accumulator with groups: every refusal (a second attach among them) leaves it as it was: one more sample, still the plain result
    acc = dev.accumulator(w, h, seed=SEED, light_groups=dict(material_group=mg, background=bg))
    level = 0
    for what, d in dict(bad, **{"a second attach": desc(), "a second attach, fewer groups": desc(n_groups=8)}).items():
        assert lib.rt_accum_attach_light_groups(acc._h, C.byref(d)) == 1, what
        assert b"rt_accum_attach_light_groups" in lib.rt_last_error(), what
        acc.render(1)
        level += 1
        check(acc, level, f"after the refusal of {what}")
    assert lib.rt_accum_attach_light_groups(acc._h, None) == 1
    reads = {
        "read into NULL": lambda: lib.rt_accum_read_light_groups(acc._h, None),
        "group == G": lambda: lib.rt_accum_resolve_light_group(acc._h, 3, 0, vp(f32)),
        "group far above": lambda: lib.rt_accum_resolve_light_group(acc._h, 0xFFFFFFFF, 0, vp(f32)),
        "group image into NULL": lambda: lib.rt_accum_resolve_light_group(acc._h, 0, 0, None),
        "group image, unknown flag": lambda: lib.rt_accum_resolve_light_group(acc._h, 0, 2, vp(f32)),
        "mix without weights": lambda: lib.rt_accum_resolve_light_mix(acc._h, None, 0, vp(f32)),
        "mix into NULL": lambda: lib.rt_accum_resolve_light_mix(acc._h, abi.fptr(wts), 0, None),
        "mix, unknown flag": lambda: lib.rt_accum_resolve_light_mix(acc._h, abi.fptr(wts), 4, vp(f32)),
        "rgb8 mix without weights": lambda: lib.rt_accum_resolve_light_mix_rgb8(acc._h, None, 0, vp(u8)),
        "rgb8 mix into NULL": lambda: lib.rt_accum_resolve_light_mix_rgb8(acc._h, abi.fptr(wts), 0, None),
        "rgb8 mix, unknown flag": lambda: lib.rt_accum_resolve_light_mix_rgb8(acc._h, abi.fptr(wts), 2, vp(u8)),
        "NULL accumulator": lambda: lib.rt_accum_resolve_light_mix(None, abi.fptr(wts), 0, vp(f32)),
    }
    for what, call in reads.items():
        assert call() == 1, what
        acc.render(1)
        level += 1
        check(acc, level, f"after the refused {what}")
    assert lib.rt_accum_resolve_light_group(acc._h, 2, 0, vp(f32)) == 0
    acc.close()

    # a fresh accumulator: the same refusals, every read refused meanwhile, then a valid attach still works
    fresh = dev.accumulator(w, h, seed=SEED)
    for what, d in bad.items():
        assert lib.rt_accum_attach_light_groups(fresh._h, C.byref(d)) == 1, what
        assert lib.rt_accum_read_light_groups(fresh._h, abi.fptr(f32)) == 1, what
    fresh.attach_light_groups(mg, background=bg)
    fresh.render(3)
    check(fresh, 3, "fresh accumulator after the refusals")
    fresh.close()

    # an accumulator that holds samples takes no groups, and one without groups refuses the reads, before and after
    late = dev.accumulator(w, h, seed=SEED)

    def reads_refused():
        assert lib.rt_accum_read_light_groups(late._h, abi.fptr(f32)) == 1
        assert lib.rt_accum_resolve_light_group(late._h, 0, 0, vp(f32)) == 1
        assert lib.rt_accum_resolve_light_mix(late._h, abi.fptr(wts), 0, vp(f32)) == 1
        assert lib.rt_accum_resolve_light_mix_rgb8(late._h, abi.fptr(wts), 0, vp(u8)) == 1

    reads_refused()
    late.render(1)
    assert lib.rt_accum_attach_light_groups(late._h, C.byref(desc())) == 1
    with pytest.raises(gpu.RtError) as e:
        late.attach_light_groups(mg, background=bg)
    assert e.value.code == 1
    reads_refused()
    late.render(1)
    r = late.read()
    assert np.all(r["samples"] == 2) and lg.same_bits(r["sum"], plain_at(2))
    late.close()
    with pytest.raises(gpu.RtError):
        dev.accumulator(w, h, seed=SEED, light_groups=dict(material_group=mg, background=7, n_groups=3))
    plain.close()
    dev.close()


# ------------------------------------------------------------------------------------------------ 8: the CLI
def test_cli_light_groups(gpu, sg, room, tmp_path):
    path = sg.write_gltf(room.sc, str(tmp_path / "room.gltf"))
    out = tmp_path / "img.ppm"
    env = dict(os.environ, RT_SEED=str(SEED), RT_DEVICE="0")
    subprocess.check_call([os.path.join(ROOT, "run.sh"), path, str(W), str(H), str(N), str(out)], env=dict(env, RT_LIGHT_GROUPS="material"))
    ls = gpu.load_scene(path, W / H)
    a = ls.arrays()
    emissive = [bool(np.any(np.asarray(m["emission"]) != 0)) for m in a["materials"]]
    assert sum(emissive) == 2
    mg, g = [], 0
    for e in emissive:  # each emissive material its own group, in material order; the background last
        mg.append(g if e else None)
        g += int(e)
    dev = gpu.DeviceScene(ls)
    acc = dev.accumulator(W, H, seed=SEED, light_groups=dict(material_group=mg, background=g, n_groups=g + 1))
    acc.render(N)

    def pixels(p):
        return np.frombuffer(p.read_bytes()[-W * H * 3:], dtype=np.uint8).reshape(H, W, 3)

    assert np.array_equal(pixels(out), acc.image(rgb8=True))
    for k in range(g + 1):
        assert np.array_equal(pixels(tmp_path / f"img_group_{k}.ppm"), gpu.tonemap(acc.light_group(k))), k
    assert all(pixels(tmp_path / f"img_group_{k}.ppm").any() for k in range(g + 1))  # each light material and the loader's white background
    assert not (tmp_path / f"img_group_{g + 1}.ppm").exists()
    acc.close()
    dev.close()
    # more than eight groups: a message, no image
    many = copy.deepcopy(room.sc)
    for m in many.materials[2:9]:
        m.emission, m.emissive_strength = (0.1, 0.1, 0.1), 1.0
    many_path = sg.write_gltf(many, str(tmp_path / "many.gltf"))
    r = subprocess.run([os.path.join(ROOT, "run.sh"), many_path, str(W), str(H), "1", str(tmp_path / "many.ppm")], env=dict(env, RT_LIGHT_GROUPS="material"),
                       capture_output=True, text=True)
    assert r.returncode != 0 and "RT_LIGHT_GROUPS" in r.stderr and not (tmp_path / "many.ppm").exists()
