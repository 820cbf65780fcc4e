"""The sentences of the accumulators' refusals (include/rt_abi.h rt_accum_*): every refusal that needs a live accumulator, as one table of
(call, the complete rt_last_error() text). The other GPU tests check the codes and the function names; callers and logs see the sentences, so
a change of the host files must leave each of them byte for byte. Every call of the table returns before anything is launched."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 8, 6
INVALID_ARG = 1  # RT_ERR_INVALID_ARG: the code of every refusal below
NO_FEATURES = "the accumulator was created without RT_ACCUM_FEATURES"
NO_IDS = "the accumulator has no ids (rt_accum_attach_ids)"
NO_GROUPS = "the accumulator has no light groups (rt_accum_attach_light_groups)"
FLAGS = "flags other than RT_FLAG_DEVICE_FB"


def _table(gpu, sc, plain, feat, ids, grp):
    """`plain` has no layer and holds samples; `feat` was created with features, `ids` has ids, `grp` two light groups; none of the three holds samples."""
    lib, abi = gpu.lib(), gpu._ctypes_abi
    DEV, OTHER = abi.RT_FLAG_DEVICE_FB, abi.RT_FLAG_COUNTERS  # the flag the reads take, and one they do not
    n_mats, n_table = len(sc.materials), sc.positions.shape[0] + len(sc.primitives)
    buf = (C.c_float * (3 * W * H * 2))()
    out = C.cast(buf, C.c_void_p)
    u32 = C.cast(buf, abi.c_u32_p)
    mats = (C.c_uint32 * n_mats)(*([0] * n_mats))
    T = []

    def add(text, call):
        T.append((text, call))

    # ---- rt_accum_render, rt_accum_render_adaptive
    def params(w=W, h=H, samples=1, flags=0):
        return abi.RtParams(w, h, samples, abi.RT_RNG_DEVICE, 0, 0, 1, 0, flags)

    def render(p):
        return lambda: lib.rt_accum_render(plain._h, C.byref(p), None)

    def adaptive(p, ad):
        return lambda: lib.rt_accum_render_adaptive(plain._h, C.byref(p), C.byref(ad) if ad is not None else None, None, None)

    ok = abi.RtAdaptive(0.1, 16, 64, 16)
    for fn, run in (("rt_accum_render", render), ("rt_accum_render_adaptive", lambda p: adaptive(p, ok))):
        add(f"{fn}: params size 7x6 differs from the accumulator's 8x6", run(params(w=7)))
        add(f"{fn}: params size 8x5 differs from the accumulator's 8x6", run(params(h=5)))
        add(f"{fn}: unknown flag, or one that does not apply to accumulators", run(params(flags=DEV)))
    add("rt_accum_render: samples must be >= 1", render(params(samples=0)))
    A = "rt_accum_render_adaptive: "
    add(A + "null argument", adaptive(params(), None))
    for t in (-1.0, float("inf"), float("nan")):
        add(A + "threshold must be finite and >= 0", adaptive(params(), abi.RtAdaptive(t, 16, 64, 16)))
    for mn, mx in ((1, 64), (16, 8), (0, 15)):
        add(A + "min_samples must be 0 or >= 2, and max_samples >= min_samples", adaptive(params(), abi.RtAdaptive(0.1, mn, mx, 16)))
    bad = abi.RtAdaptive(0.1, 16, 64, 16)
    bad.reserved[3] = 1
    add(A + "reserved fields must be 0", adaptive(params(), bad))

    # ---- rt_accum_resolve, rt_accum_resolve_rgb8
    for fn in ("rt_accum_resolve", "rt_accum_resolve_rgb8"):
        f = getattr(lib, fn)
        add(f"{fn}: null argument or {FLAGS}", lambda f=f: f(plain._h, OTHER, out))
        add(f"{fn}: null argument or {FLAGS}", lambda f=f: f(plain._h, 0, None))

    # ---- features and the denoiser
    add(f"rt_accum_read_features: {NO_FEATURES}", lambda: lib.rt_accum_read_features(plain._h, buf, buf, buf, u32))
    add(f"rt_accum_resolve_features: {NO_FEATURES}", lambda: lib.rt_accum_resolve_features(plain._h, 0, out, out, out))
    add(f"rt_accum_resolve_features: {FLAGS}", lambda: lib.rt_accum_resolve_features(feat._h, DEV | OTHER, out, out, out))
    for fn in ("rt_accum_denoise", "rt_accum_denoise_rgb8"):
        f = getattr(lib, fn)

        def den(f=f, acc=feat, call_flags=0, dst=out, **fields):
            o = abi.RtDenoise()
            for k, v in fields.items():
                if k == "reserved":
                    o.reserved[v] = 1
                else:
                    setattr(o, k, v)
            return lambda: f(acc._h, C.byref(o), call_flags, dst)

        add(f"{fn}: {NO_FEATURES}", den(acc=plain))
        add(f"{fn}: null buffer or {FLAGS}", den(dst=None))
        add(f"{fn}: null buffer or {FLAGS}", den(call_flags=OTHER))
        for k in range(3):
            add(f"{fn}: reserved fields must be 0", den(reserved=k))
        for fields in (dict(iterations=9), dict(normal_sharpness=9), dict(flags=2)):
            add(f"{fn}: iterations and normal_sharpness are at most 8; unknown rt_denoise.flags bit", den(**fields))
        for fields in (dict(sigma_color=-1.0), dict(sigma_color=float("inf")), dict(sigma_depth=float("nan")), dict(sigma_depth=float("inf"))):
            add(f"{fn}: sigma_color and sigma_depth must be finite and >= 0", den(**fields))

    # ---- ids
    add(f"rt_accum_read_ids: {NO_IDS}", lambda: lib.rt_accum_read_ids(plain._h, u32, u32, u32))
    add(f"rt_accum_resolve_labels: {NO_IDS}", lambda: lib.rt_accum_resolve_labels(plain._h, 0, out, out))
    add(f"rt_accum_resolve_matte: {NO_IDS}", lambda: lib.rt_accum_resolve_matte(plain._h, 0, u32, 1, out))
    add(f"rt_accum_resolve_labels: {FLAGS}", lambda: lib.rt_accum_resolve_labels(ids._h, OTHER, out, out))
    M = f"rt_accum_resolve_matte: null ids or matte, n_ids outside 1..4096, or {FLAGS}"
    add(M, lambda: lib.rt_accum_resolve_matte(ids._h, 0, None, 1, out))
    add(M, lambda: lib.rt_accum_resolve_matte(ids._h, 0, u32, 1, None))
    add(M, lambda: lib.rt_accum_resolve_matte(ids._h, 0, u32, 0, out))
    add(M, lambda: lib.rt_accum_resolve_matte(ids._h, 0, u32, 4097, out))
    add(M, lambda: lib.rt_accum_resolve_matte(ids._h, OTHER, u32, 1, out))

    def attach_ids(acc, kind=abi.RT_ID_PRIMITIVE, slots=0, table=None, n=0, flags=0, reserved=None):
        d = abi.RtIdDesc()
        d.kind, d.slots, d.table, d.n_table, d.flags = kind, slots, table, n, flags
        if reserved is not None:
            d.reserved[reserved] = 1
        return lambda: lib.rt_accum_attach_ids(acc._h, C.byref(d))

    I = "rt_accum_attach_ids: "
    add(I + "null argument", lambda: lib.rt_accum_attach_ids(feat._h, None))
    add(I + "unknown kind 3", attach_ids(feat, kind=3))
    add(I + "slots must be 0 (= 4) or 1..16", attach_ids(feat, slots=17))
    for kw in (dict(reserved=0), dict(reserved=1), dict(flags=OTHER)):
        add(I + f"reserved fields must be 0; {FLAGS}", attach_ids(feat, **kw))
    for kw in (dict(), dict(table=C.addressof(buf), n=n_table + 1)):
        add(I + f"RT_ID_USER needs a table of n_triangles + n_primitives = {n_table} ids", attach_ids(feat, kind=abi.RT_ID_USER, **kw))
    add(I + "only RT_ID_USER takes a table", attach_ids(feat, kind=abi.RT_ID_MATERIAL, table=C.addressof(buf)))
    add(I + "only RT_ID_USER takes a table", attach_ids(feat, n=1))
    add(I + "the device table must be 4-byte aligned", attach_ids(feat, kind=abi.RT_ID_USER, table=C.addressof(buf) + 2, n=n_table, flags=DEV))
    add(I + "the accumulator already has ids", attach_ids(ids))
    add(I + "the accumulator already holds samples; attach ids before the first render", attach_ids(plain))

    # ---- light groups
    w = C.cast(buf, abi.c_float_p)
    add(f"rt_accum_read_light_groups: {NO_GROUPS}", lambda: lib.rt_accum_read_light_groups(plain._h, w))
    add(f"rt_accum_resolve_light_group: {NO_GROUPS}", lambda: lib.rt_accum_resolve_light_group(plain._h, 0, 0, out))
    add(f"rt_accum_read_light_groups: null buffer or {FLAGS}", lambda: lib.rt_accum_read_light_groups(grp._h, None))
    add(f"rt_accum_resolve_light_group: null buffer or {FLAGS}", lambda: lib.rt_accum_resolve_light_group(grp._h, 0, 0, None))
    add(f"rt_accum_resolve_light_group: null buffer or {FLAGS}", lambda: lib.rt_accum_resolve_light_group(grp._h, 0, OTHER, out))
    add("rt_accum_resolve_light_group: group 2 of 2", lambda: lib.rt_accum_resolve_light_group(grp._h, 2, 0, out))
    add("rt_accum_resolve_light_group: group 4294967295 of 2", lambda: lib.rt_accum_resolve_light_group(grp._h, 0xFFFFFFFF, DEV, out))
    for fn in ("rt_accum_resolve_light_mix", "rt_accum_resolve_light_mix_rgb8"):
        f = getattr(lib, fn)
        add(f"{fn}: {NO_GROUPS}", lambda f=f: f(plain._h, w, 0, out))
        add(f"{fn}: null buffer or {FLAGS}", lambda f=f: f(grp._h, w, 0, None))
        add(f"{fn}: null buffer or {FLAGS}", lambda f=f: f(grp._h, w, OTHER, out))
        add(f"{fn}: null weights", lambda f=f: f(grp._h, None, 0, out))

    def attach_groups(acc, n_groups=2, background=abi.RT_LIGHT_GROUP_NONE, table=C.addressof(mats), n=n_mats, flags=0, reserved=None):
        d = abi.RtLightGroupDesc()
        d.n_groups, d.background_group, d.material_group, d.n_materials, d.flags = n_groups, background, table, n, flags
        if reserved is not None:
            d.reserved[reserved] = 1
        return lambda: lib.rt_accum_attach_light_groups(acc._h, C.byref(d))

    G = "rt_accum_attach_light_groups: "
    add(G + "null argument", lambda: lib.rt_accum_attach_light_groups(feat._h, None))
    for g in (0, 9):
        add(G + "n_groups must be 1..8", attach_groups(feat, n_groups=g))
    for kw in (dict(reserved=0), dict(reserved=1), dict(flags=OTHER)):
        add(G + f"reserved fields must be 0; {FLAGS}", attach_groups(feat, **kw))
    for kw in (dict(table=None), dict(n=n_mats + 1)):
        add(G + f"material_group must hold the scene's {n_mats} materials", attach_groups(feat, **kw))
    add(G + "the device table must be 4-byte aligned", attach_groups(feat, table=C.addressof(mats) + 1, flags=DEV))
    add(G + "background_group must be below n_groups, or RT_LIGHT_GROUP_NONE", attach_groups(feat, background=2))
    add(G + "the accumulator already has light groups", attach_groups(grp))
    add(G + "the accumulator already holds samples; attach light groups before the first render", attach_groups(plain))
    far = (C.c_uint32 * n_mats)(*([0] * (n_mats - 1) + [2]))  # checked on the host, after the two refusals above
    add(G + f"material_group[{n_mats - 1}] is neither below n_groups nor RT_LIGHT_GROUP_NONE", attach_groups(feat, table=C.addressof(far)))
    return T, (buf, mats, far)


def test_every_refusal_of_a_live_accumulator_says_its_sentence(gpu, scenes):
    sc = scenes["open_nolight"]  # the smallest room of the fixtures
    dev = gpu.DeviceScene(sc)  # the parity build
    plain = dev.accumulator(W, H)
    feat = dev.accumulator(W, H, features=True)
    ids = dev.accumulator(W, H, ids="primitive")
    grp = dev.accumulator(W, H, light_groups=dict(material_group=[0] * len(sc.materials), background=1))
    plain.render(1)  # it holds samples: the late attaches
    before = plain.read()
    lib = gpu.lib()
    table, keep = _table(gpu, sc, plain, feat, ids, grp)
    assert len(table) == 98
    wrong = []
    for k, (text, call) in enumerate(table):
        rc = call()
        got = lib.rt_last_error().decode()
        print(f"{k:3d} rc={rc} {got}")
        if rc != INVALID_ARG or got != text:
            wrong.append((k, rc, got, text))
    assert wrong == []
    # the refused accumulators are as they were: still without samples or layers of their own beyond what they were made with
    after = plain.read()
    assert all(np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)) for k in before)
    assert np.all(feat.read()["samples"] == 0) and np.all(ids.read()["samples"] == 0) and np.all(grp.read()["samples"] == 0)
    with pytest.raises(gpu.RtError):
        feat.read_ids()
    with pytest.raises(gpu.RtError):
        feat.read_light_groups()
    assert grp.n_light_groups == 2 and ids.id_slots == 4
    del keep
    dev.close()
