"""Ray sets built to leave the exact-reciprocal-division fast path (csrc/rt_dev_trav.h, div_exact_fast): a direction component outside
[2^-40, 2^40] or an origin component that is neither 0 nor within [2^-37, 2^40] sends a ray through the reference's IEEE division.
Shared by tests/test_gpu_parity.py (the per-lane probe) and tests/test_gpu_production.py (every binary closest-hit kernel)."""
import numpy as np

from conftest import random_rays


def degenerate_rays(sc):
    """Axis-parallel rays from points ON box planes / vertices: 0/0 and +-inf slab terms (bvh.h:141-145). 6 x 300 rays."""
    verts = sc.positions.reshape(-1, 3)[:300]
    rays = []
    for ax in range(3):
        for sgn in (-1.0, 1.0):
            d = np.zeros(3, dtype=np.float32)
            d[ax] = sgn
            for v in verts:
                rays.append(np.concatenate([v + np.float32(0.0), d]))
    return np.asarray(rays, dtype=np.float32)


def fast_division_boundary_rays(sc):
    """6000 rays on both sides of the fast path's preconditions: origin components that are 0, tiny (1e-30), huge (1e15); direction
    components that are 0, 1e-20 or dominate."""
    rays = random_rays(sc, 6000, seed=303)
    rng = np.random.default_rng(8)
    specials_o = np.array([0.0, 1e-30, -1e-30, 1e-13, 1e15, 4.0, -20.0, 16.0], dtype=np.float32)
    specials_d = np.array([0.0, 1e-20, -1e-20, 1e-13, 1.0], dtype=np.float32)
    for i in range(3000):
        rays[i, rng.integers(0, 3)] = rng.choice(specials_o)
        if i % 2:
            rays[i, 3 + rng.integers(0, 3)] = rng.choice(specials_d)
    return rays


def big_leaf_scene(sg):
    """Many triangles with identical centroids: the SAH sweep finds no split (bvh.h:299-312), so a leaf holds dozens of triangles (beyond
    RT_LEAF_COOP_MAX: walked triangle by triangle) and equal-t hits occur."""
    sc = sg.boxes_scene(n_boxes=5, seed=8, n_lights=2)
    tri = sc.positions[20:21]
    dup = np.repeat(tri, 40, axis=0)
    sc.positions = np.concatenate([sc.positions, dup, dup * np.float32(1.0)], axis=0).astype(np.float32)
    n = sc.positions.shape[0]
    sc.material_ids = np.concatenate([sc.material_ids, np.full(80, 3, dtype=np.uint32)])
    sc.texcoords = np.zeros((n, 3, 2), dtype=np.float32)
    sc.tangents = np.zeros((n, 3, 3), dtype=np.float32)
    sc.tangents[..., 0] = 1
    return sc


def is_guarded(rays):
    """The per-ray half of the fast path's preconditions, negated (ray_fast_ok_ray)."""
    o, d = rays[:, :3], np.abs(rays[:, 3:])
    lo, hi, olo = np.float32(2.0**-40), np.float32(2.0**40), np.float32(2.0**-37)
    d_ok = (d >= lo).all(axis=1) & (d <= hi).all(axis=1)
    m = np.abs(o)
    o_ok = ((o == 0) | ((m >= olo) & (m <= hi))).all(axis=1)
    return ~(d_ok & o_ok)
