"""Fixtures and comparisons for the light groups of an accumulator (include/rt_abi.h, rt_accum_attach_light_groups). A plain module next to the
tests (imported like adaptive_replay.py).

The exact check rests on one property of the fold: it never mixes colour channels. In a scene whose first group of emitters is red only, whose
second is green only and whose background is blue only, group g's sum must be, bit for bit, channel g of the ungrouped sum S and zero in the
other two channels. `channel_scene` makes such a scene of a golden scene: a copy of material 1 (the lights) is appended, every second light
triangle moves to the copy, the two emit (1, 0, 0) and (0, 0.9, 0) at the strength the scene had, the background is (0, 0, 0.7). `plain_scene`
is the same split with ordinary colours: the same triangles, light tree and paths (test_light_group_fixtures.py asserts that)."""
import copy

import numpy as np

NONE = 0xFFFFFFFF
W, H, N, SEED = 64, 48, 8, 7
COUNTERS = ("samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests",
            "light_tri_tests", "light_hits", "texel_fetches")
CENSUS_SLOTS = ("shade_alpha_pass", "shade_p_lt_eps_exit", "shade_scl_zero_exit", "shade_push", "trace_miss_background", "trace_depth_exhausted")


def split_lights(scene, parts=2):
    """A deep copy of `scene` with parts - 1 copies of material 1 (the lights) appended. With two parts every second light triangle,
    lights[::2] in triangle order, moves to the copy; with more, lights[k - 1::parts] move to copy k and the rest keep material 1.
    Returns (scene, [material 1, the copies])."""
    sc = copy.deepcopy(scene)
    lights = np.nonzero(sc.material_ids == 1)[0]
    assert len(lights) >= parts
    mats = [1]
    for _ in range(parts - 1):
        sc.materials.append(copy.deepcopy(sc.materials[1]))
        mats.append(len(sc.materials) - 1)
    sc.material_ids = sc.material_ids.copy()
    if parts == 2:
        sc.material_ids[lights[::2]] = mats[1]
    else:
        for k in range(1, parts):
            sc.material_ids[lights[k - 1::parts]] = mats[k]
    return sc, mats


def channel_scene(scene):
    """(scene, material_group, background group): red lights in group 0, green lights in group 1, a blue background in group 2."""
    sc, (m0, m1) = split_lights(scene)
    sc.materials[m0].emission = (1.0, 0.0, 0.0)
    sc.materials[m1].emission = (0.0, 0.9, 0.0)
    sc.bg_color = (0.0, 0.0, 0.7)
    mg = [None] * len(sc.materials)
    mg[m0], mg[m1] = 0, 1
    return sc, mg, 2


def plain_scene(scene):
    """channel_scene's triangles and materials with ordinary colours."""
    sc, (m0, m1) = split_lights(scene)
    sc.materials[m1].emission = (0.6, 0.8, 1.0)
    sc.bg_color = (0.3, 0.4, 0.7)
    return sc


def five_group_scene(scene):
    """Three light materials with ordinary colours, a coloured background: (scene, material_group, background group, G = 5). Group 3 is empty."""
    sc, (m0, m1, m2) = split_lights(scene, parts=3)
    sc.materials[m1].emission = (0.6, 0.8, 1.0)
    sc.materials[m2].emission = (1.0, 0.5, 0.3)
    sc.bg_color = (0.3, 0.4, 0.7)
    mg = [None] * len(sc.materials)
    mg[m0], mg[m1], mg[m2] = 0, 1, 2
    return sc, mg, 4, 5


def only_group(scene, material_group, background, g, scale=2.0 ** -100):
    """`scene` with every emitter outside group g, the background included, scaled by `scale`: a power of two, so the scaled emitters stay
    emitters (the light tree and every path are unchanged) and contribute at most `scale` times what they did."""
    sc = copy.deepcopy(scene)
    for m, grp in zip(sc.materials, material_group):
        if grp != g:
            m.emission = tuple(float(np.float32(e) * np.float32(scale)) for e in m.emission)
    if background != g:
        sc.bg_color = tuple(float(np.float32(c) * np.float32(scale)) for c in sc.bg_color)
    return sc


def fold_sum(samples, counts=None):
    """S of (..., N, 3) samples: binary32 additions in sample order from +0; `counts` (...): only the first n_p samples of each pixel."""
    x = np.asarray(samples, dtype=np.float32)
    S = np.zeros(x.shape[:-2] + (3,), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(x.shape[-2]):
            S = S + x[..., s, :] if counts is None else np.where((s < np.asarray(counts))[..., None], S + x[..., s, :], S)
    return S


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def assert_channels(GS, S, groups=(0, 1, 2), what=""):
    """The exact check: for k, g in enumerate(groups), GS[g] is channel k of S bit for bit and == 0 in the other channels (so -0 passes). A
    g of None skips that channel. Groups of GS not named must be zero everywhere."""
    GS = np.asarray(GS, dtype=np.float32)
    S = np.asarray(S, dtype=np.float32)
    assert GS.shape[1:] == S.shape, f"{what}: shapes {GS.shape} and {S.shape}"
    for k, g in enumerate(groups):
        if g is None:
            continue
        got, want = GS[g, ..., k], S[..., k]
        ok = got.view(np.uint32) == want.view(np.uint32)
        if not ok.all():
            i = tuple(int(v) for v in np.argwhere(~ok)[0])
            raise AssertionError(f"{what}: group {g} channel {k}: {int((~ok).sum())} pixels differ; first at {i}: got {got[i]!r}, want {want[i]!r}")
        for c in range(3):
            if c != k:
                assert np.all(GS[g, ..., c] == 0), f"{what}: group {g} channel {c} is not zero everywhere"
    for g in range(GS.shape[0]):
        if g not in groups:
            assert np.all(GS[g] == 0), f"{what}: group {g} holds something"


def mix_model(GS, n, weights):
    """rt_accum_resolve_light_mix restated in numpy float32: per channel acc = +0; for g ascending acc = acc + (GS_g / n) * w[g][c]; a quotient
    is 0 where n = 0."""
    w = np.asarray(weights, dtype=np.float32)
    nf = np.asarray(n).astype(np.float32)[..., None]
    acc = np.zeros(GS.shape[1:], dtype=np.float32)
    with np.errstate(all="ignore"):
        for g in range(GS.shape[0]):
            m = np.where(nf > 0, GS[g] / np.where(nf > 0, nf, np.float32(1)), np.float32(0)).astype(np.float32)
            acc = (acc + (m * w[g][None, None, :]).astype(np.float32)).astype(np.float32)
    return acc


def group_mean(GS_g, n):
    nf = np.asarray(n).astype(np.float32)[..., None]
    with np.errstate(all="ignore"):
        return np.where(nf > 0, np.asarray(GS_g, np.float32) / np.where(nf > 0, nf, np.float32(1)), np.float32(0)).astype(np.float32)
