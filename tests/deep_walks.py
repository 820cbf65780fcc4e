"""Scenes and ray sets whose BVH walks keep many deferred siblings pending, so that the slow tier behind every LDS stack executes
(csrc/rt_dev_stack.h; DESIGN.md "Traversal stack: which tier a walk reaches"). Generated room scenes put a few coplanar lights under the
ceiling: a light query crosses two or three boxes there and no closest-hit ray holds more than a dozen frames. Here the lights fill the volume
with large overlapping triangles, or the scene is a soup of long needles whose boxes nearly all overlap.

Shared by tests/test_gpu_deep_walks.py, tests/test_oracle_golden.py and tests/golden/make_live_golden.py. Which tier a ray reaches is not
assumed: OracleScene.walk_census counts it, and `tier_shares` / `require_witnesses` turn the counts into the conditions the tests assert.

Pending counts f (deferred far siblings at once) and the tier they enter:
  light walk    f >= 5   wf_shade's scratch half (4 LDS positions)            f >= 13  the probe's / megakernel's scratch half (12 LDS positions)
  closest hit   f >= 8   first eviction of wf_extend's 6-deep ring            f >= 14  the probe's / megakernel's scratch half (the newest frame
                         (newest frame in registers + 6 in LDS)                        is in registers, 12 in LDS)
"""
import numpy as np

from conftest import random_rays

LIGHT_SHADE_SCRATCH = 5    # lights_pdf through StackMemT<4>: position 4 is the first in scratch
LIGHT_PROBE_SCRATCH = 13   # lights_pdf through StackMemT<12>
CLOSEST_RING_EVICT = 8     # wf_extend: registers + RingStackT<6>; the 8th pending frame evicts the oldest
CLOSEST_PROBE_SCRATCH = 14 # cast_kernel / megakernel: registers + StackMemT<12>; the 14th pending frame goes to scratch

# the two generated scenes every deep-walk test and stored answer uses
BIG_LIGHTS = dict(n_lights=2000, size=6.0, seed=31)
NEEDLES = dict(n=20000, seed=41)
# light counts on both sides of wf_shade's staging rule (inner nodes + lights <= 96 is staged in LDS), found by counting the trees these
# parameters build (tests/test_oracle_golden.py pins the sums without a GPU)
STAGING_EDGE = {96: dict(n_lights=77, size=3.0, seed=5), 97: dict(n_lights=78, size=3.0, seed=6)}


def _append(sg, sc, tri, material_id, rng):
    n = len(tri)
    tri = tri.astype(np.float32) + np.float32(0.0)
    tex = np.zeros((n, 3, 2), dtype=np.float32)
    if sc.textures:
        tex = (rng.uniform(0, 4, size=(n, 1, 2)) + rng.uniform(-0.3, 0.3, size=(n, 3, 2))).astype(np.float32)
    tan = np.zeros((n, 3, 3), dtype=np.float32)
    tan[..., 0] = 1.0
    ids = np.full(n, material_id, dtype=np.uint32) if np.ndim(material_id) == 0 else np.asarray(material_id, dtype=np.uint32)
    sc.positions = np.concatenate([sc.positions, tri]).astype(np.float32)
    sc.texcoords = np.concatenate([sc.texcoords, tex]).astype(np.float32)
    sc.tangents = np.concatenate([sc.tangents, tan]).astype(np.float32)
    sc.material_ids = np.concatenate([sc.material_ids, ids]).astype(np.uint32)
    assert sc.normals is None
    return sc


def volume_lights_scene(sg, n_lights, size, seed, n_random=300, n_materials=4, textured=False, strength=0.5, env_texture=None):
    """A small closed room (scenegen.room_scene with no ceiling lights, `n_random` small random triangles, `n_materials` materials, textured
    with 8x8 texture sets on request) plus `n_lights` emissive triangles with centres uniform in the room and vertex offsets uniform in
    +-`size`, clipped inside the walls (one that the clipping leaves without area is drawn again): the light tree's boxes overlap
    throughout the volume. The room is drawn with `seed`, the lights with `seed + 1`. `strength`: emission of the lights (modest: with thousands of them every path meets several). `env_texture`: an (H, W, 4)
    uint8 picture that becomes the environment map; the room is then built open, so that paths reach it."""
    sc = sg.room_scene(n_random, seed=seed, n_lights=0, n_materials=n_materials, tex_size=8 if textured else 0, n_tex_sets=2, light_strength=strength,
                       alpha_fraction=0.1, open_room=env_texture is not None)
    rng = np.random.default_rng(seed + 1)
    lo, hi = np.array([-20.0, 0.0, -10.0], dtype=np.float32), np.array([20.0, 16.0, 10.0], dtype=np.float32)

    def draw(k):
        cen = rng.uniform(lo + 0.3, hi - 0.3, size=(k, 1, 3))
        return np.clip(cen + rng.uniform(-size, size, size=(k, 3, 3)), lo + 0.01, hi - 0.01)

    tri = draw(n_lights)
    while True:  # three vertices clipped onto one edge of the room make a triangle without area: draw those again
        flat = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) < 1e-3
        if not flat.any():
            break
        tri[flat] = draw(int(flat.sum()))
    _append(sg, sc, tri, 1, rng)  # material 1: room_scene's light material
    if env_texture is not None:
        sc.textures = list(sc.textures) + [np.ascontiguousarray(env_texture, dtype=np.uint8)]
        sc.bg_texture = len(sc.textures) - 1
    return sc


def needle_soup_scene(sg, n, seed, half_length=(3.0, 10.0), width=0.02, emissive=False, strength=0.05, n_ceiling_lights=4):
    """A closed room plus `n` long thin triangles: centres uniform in the room, random axes, half-lengths uniform in `half_length`, `width`
    wide (they may poke through the walls). Nearly every needle's box holds a large part of the room, so the SAH tree's boxes overlap at every
    level and a walk defers a sibling at most of them. emissive=True: the needles are the lights (the light tree is the deep one, no ceiling
    lights); otherwise they take the room's materials and `n_ceiling_lights` ordinary lights hang under the ceiling."""
    sc = sg.room_scene(0, seed=seed, n_lights=0 if emissive else n_ceiling_lights, n_materials=4, tex_size=0, light_strength=strength if emissive else 8.0)
    rng = np.random.default_rng(seed + 1)
    lo, hi = np.array([-20.0, 0.0, -10.0]), np.array([20.0, 16.0, 10.0])
    cen = rng.uniform(lo + 0.3, hi - 0.3, size=(n, 3))
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    side = np.cross(axis, rng.normal(size=(n, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    half = rng.uniform(half_length[0], half_length[1], size=(n, 1))
    tri = np.stack([cen - half * axis, cen + half * axis, cen + width * side], axis=1)
    ids = 1 if emissive else rng.integers(2, 6, size=n)
    return _append(sg, sc, tri, ids, rng)


def light_triangles(sc):
    return np.array([i for i, m in enumerate(sc.material_ids) if any(e != 0 for e in sc.materials[int(m)].emission_f32())], dtype=np.int64)


def light_query_rays(sc, n, seed):
    """conftest.random_rays with the first half aimed at light centroids (as test_light_pdf_bit_exact does), so that the sums are not empty."""
    rays = random_rays(sc, n, seed=seed)
    cen = sc.positions[light_triangles(sc)].mean(axis=1)
    tgt = cen[np.random.default_rng(seed + 1).integers(0, len(cen), size=n // 2)]
    d = tgt - rays[: len(tgt), :3]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays[: len(tgt), 3:] = d.astype(np.float32)
    return rays


def long_diagonal_rays(sc, n, seed):
    """Rays from one end wall of the room to the other (x = -19.5 -> 19.5, random y and z at both ends): they cross the whole volume, where a
    volume-light scene is densest along a ray."""
    rng = np.random.default_rng(seed)
    a = np.stack([np.full(n, -19.5), rng.uniform(0.5, 15.5, n), rng.uniform(-9.5, 9.5, n)], axis=1)
    b = np.stack([np.full(n, 19.5), rng.uniform(0.5, 15.5, n), rng.uniform(-9.5, 9.5, n)], axis=1)
    d = b - a
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([a, d], axis=1).astype(np.float32)


def inner_plus_lights(info):
    """`inner + lights` of a light tree's bvh_info: what the staging rule of wf_shade counts (csrc/rt_scene.cpp light_lds_inner)."""
    nodes = info["nodes"]
    return int((nodes[:, 6] != 0xFFFFFFFF).sum()) + len(info["order"])


def tier_shares(counts, thresholds):
    """{threshold: share of the rays whose pending count reaches it} and the maximum count."""
    counts = np.asarray(counts)
    return {int(t): float((counts >= t).mean()) for t in thresholds}, int(counts.max(initial=0))


def require_witnesses(what, counts, required):
    """Assert that the rays reach every tier a test claims: `required` maps a pending count to the least share of the rays that must reach
    it. Prints the measured shares and the maximum (the tests run with -s where a report is wanted); returns them."""
    shares, most = tier_shares(counts, required.keys())
    print(f"[deep walks] {what}: most pending {most}; " + ", ".join(f"{100 * s:.1f} % of {len(counts)} rays reach f >= {t}" for t, s in shares.items()))
    for t, need in required.items():
        assert shares[int(t)] >= need, f"{what}: only {100 * shares[int(t)]:.2f} % of the rays keep {t} siblings pending, the test needs {100 * need:.0f} %"
    return shares, most
