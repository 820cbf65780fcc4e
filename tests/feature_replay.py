"""A host model of the first-hit feature sums of a feature accumulator (include/rt_abi.h, RT_ACCUM_FEATURES), for exact comparisons with the
device. A plain module next to the tests (imported like adaptive_replay.py). It needs no oracle code of its own:
  primary_rays   the first ray of every sample of every pixel, from OracleScene.trace_pixel (the ray seeded from (seed, p, s));
  first_hits     OracleScene.cast_rays on those rays: hit flags and t;
  twin_scene     the same geometry, camera and textures with emission := color.rgb, emissive_tex := color_tex, colour alpha 1, a black
                 background and ray_depth 1. Under ray_depth 1 shade() returns emission + 0 * scl, so the oracle's pixel_samples of the twin are
                 material.color.rgb x colour texel of the closest primary hit and 0 on a miss: the operands and products of the albedo. The twin
                 needs texture alpha 1 wherever a primary ray lands (twin_alpha_is_one checks the whole texture set);
  ladder         binary32 additions in sample order from +0.0, every prefix kept: level L holds the sums of samples 0 .. L - 1."""
import dataclasses

import numpy as np

NONE = 0xFFFFFFFF


def primary_rays(orc, w, h, n, seed, pixels=None):
    """(P, n, 6) float32: the primary ray of samples 0 .. n - 1 of each pixel (all w * h pixels by default)."""
    pixels = np.arange(w * h) if pixels is None else np.asarray(pixels)
    out = np.zeros((len(pixels), n, 6), dtype=np.float32)
    for i, p in enumerate(pixels):
        rays, smp = orc.trace_pixel(w, h, n, int(p), seed=seed)
        s, first = np.unique(smp, return_index=True)  # cast order: the first ray a sample casts is its primary ray
        assert np.array_equal(s, np.arange(n)), f"pixel {p}: samples {s.tolist()} cast rays"
        out[i] = rays[first]
    return out


def first_hits(orc, rays):
    """(hit (P, n) bool, t (P, n) float32 with 0 for a miss, prim (P, n) uint32) of OracleScene.cast_rays."""
    prim, bct = orc.cast_rays(rays.reshape(-1, 6))
    hit = prim != NONE
    assert not bct[~hit].any()
    return hit.reshape(rays.shape[:2]), bct[:, 2].reshape(rays.shape[:2]).copy(), prim.reshape(rays.shape[:2])


def twin_scene(sc):
    """The twin of a scenegen.Scene (see the module docstring)."""
    mats = [dataclasses.replace(m, color=(m.color[0], m.color[1], m.color[2], 1.0), emission=tuple(m.color[:3]), emissive_strength=None,
                                emissive_tex=m.color_tex) for m in sc.materials]
    return dataclasses.replace(sc, materials=mats, bg_color=(0.0, 0.0, 0.0), ray_depth=1)


def twin_alpha_is_one(sc):
    """Every texture a material uses as its colour texture has alpha 255 in every texel: no primary hit of the twin can pass through."""
    return all(m.color_tex < 0 or bool((np.asarray(sc.textures[m.color_tex])[..., 3] == 255).all()) for m in sc.materials)


def ladder(x):
    """x (P, n) or (P, n, 3) -> (n + 1, P[, 3]) float32: the sequential binary32 sum of every prefix."""
    x = np.asarray(x, dtype=np.float32)
    acc = [np.zeros(x.shape[:1] + x.shape[2:], dtype=np.float32)]
    for s in range(x.shape[1]):
        acc.append(acc[-1] + x[:, s])  # one addition per sample (np.sum would add pairwise)
    return np.stack(acc)


def hit_ladder(hit):
    return np.concatenate([np.zeros((1, hit.shape[0]), np.uint32), np.cumsum(hit, axis=1, dtype=np.uint32).T])


def at(lad, n):
    """Level n_p of a ladder (L + 1, P, ...) for every pixel: n (H, W) -> (H, W, ...)."""
    n = np.asarray(n).astype(np.int64)
    flat = lad[n.reshape(-1), np.arange(n.size)]
    return flat.reshape(n.shape + lad.shape[2:])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ; first at {i}: got {got[i]!r}, want {want[i]!r}")


def geometric_normals_f64(sc, rays, prim, hit):
    """+-normalize(cross(b - a, c - a)) of each ray's hit triangle in float64, facing the ray; 0 for a miss. rays (..., 6), prim, hit (...)."""
    pos = np.asarray(sc.positions, dtype=np.float64)
    k = np.where(hit, prim, 0).astype(np.int64)
    a, b, c = pos[k, 0], pos[k, 1], pos[k, 2]
    g = np.cross(b - a, c - a)
    g /= np.linalg.norm(g, axis=-1, keepdims=True)
    away = (g * rays[..., 3:6].astype(np.float64)).sum(-1) > 0
    g = np.where(away[..., None], -g, g)
    return np.where(hit[..., None], g, 0.0)
