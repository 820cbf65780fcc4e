"""Scenes and ray sets whose BVH walks keep many deferred siblings pending, so that the slow tier behind every LDS stack executes
(csrc/rt_dev_stack.h; DESIGN.md "Traversal stack: which tier a walk reaches"). Generated room scenes put a few coplanar lights under the
ceiling: a light query crosses two or three boxes there and no closest-hit ray holds more than a dozen frames. Here the lights fill the volume
with large overlapping triangles, or the scene is a soup of long needles whose boxes nearly all overlap.

Shared by tests/test_gpu_deep_walks.py, tests/test_oracle_golden.py and tests/golden/make_live_golden.py. Which tier a ray reaches is not
assumed: OracleScene.walk_census counts it, and `tier_shares` / `require_witnesses` turn the counts into the conditions the tests assert.
The second half of the file goes beyond what a reference-built tree can reach (19 frames): a scene that makes the device's radix tree 41 or
46 deep, and a census of the tree the device built (tests/test_gpu_deep_device_trees.py, tests/test_walk_census.py).

Pending counts f (deferred far siblings at once) and the tier they enter:
  light walk    f >= 5   wf_shade's scratch half (4 LDS positions)            f >= 13  the probe's / megakernel's scratch half (12 LDS positions)
  closest hit   f >= 8   first eviction of wf_extend's 6-deep ring            f >= 14  the probe's / megakernel's scratch half (the newest frame
                         (newest frame in registers + 6 in LDS)                        is in registers, 12 in LDS)
  8-wide walk   g >= 10  first eviction of wf_extend_wide's 8-deep ring (g counts pending node GROUPS: `wide_census`, the last part of the file)
"""
import numpy as np

from bvh_dump import LEAF, MASK, NONE
from conftest import random_rays

LIGHT_SHADE_SCRATCH = 5    # lights_pdf through StackMemT<4>: position 4 is the first in scratch
LIGHT_PROBE_SCRATCH = 13   # lights_pdf through StackMemT<12>
CLOSEST_RING_EVICT = 8     # wf_extend: registers + RingStackT<6>; the 8th pending frame evicts the oldest
CLOSEST_PROBE_SCRATCH = 14 # cast_kernel / megakernel: registers + StackMemT<12>; the 14th pending frame goes to scratch
# wf_extend_wide (csrc/rt_wide.hip): the newest pending group in registers (top_x, top_y), older ones in RingStackT<8, 2>, older still in the
# global workspace. wide_node_step spills the previous top with stk.push(sp - 1, ...) when it stacks a group at sp > 0, and push finds the ring
# full when pos - base == 8, base = 0: pos = 8 = sp - 1, so sp goes from 9 to 10. The 10th pending group is the first eviction, and every
# refill from the workspace (pop_masked with pos < base) happens on the way back from there.
WIDE_RING_EVICT = 10
WIDE_CLAIM = 12            # what the tests assert: two groups past the first eviction (why: `wide_census`)

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


def require_witnesses(what, counts, required, tag="deep walks", unit="siblings", report=()):
    """Assert that the rays reach every tier a test claims: `required` maps a pending count to the least share of the rays that must reach
    it. Prints the measured shares and the maximum (the tests run with -s where a report is wanted); returns them. `report`: further pending
    counts whose shares are printed and returned without a claim; `tag`, `unit`: the line's prefix and what is counted."""
    shares, most = tier_shares(counts, list(required.keys()) + [t for t in report if t not in required])
    print(f"[{tag}] {what}: most pending {most}; " + ", ".join(f"{100 * s:.1f} % of {len(counts)} rays reach f >= {t}" for t, s in shares.items()))
    for t, need in required.items():
        assert shares[int(t)] >= need, f"{what}: only {100 * shares[int(t)]:.2f} % of the rays keep {t} {unit} pending, the test needs {100 * need:.0f} %"
    return shares, most


# ------------------------------------------------------------------------------------------------ deep trees from the device's radix builder
# The reference builder's SAH tree cannot be made deep, so no scene above keeps more than 19 frames pending. The Karras radix tree of
# csrc/rt_bvh_device.hip (RT_BUILDER_LBVH) can: it splits at the bits of a 30-bit Morton code and, inside a run of equal codes, at the bits of
# the leaf index. `corner_ladder_scene` gives every one of the 30 code bits a split whose two boxes both hold the scene's corner, and ends the
# chain in a run of 2^log2_soup equal codes around that corner: a ray that starts there defers a sibling at every level. Which count a ray
# really reaches is read off the tree the device built (`dump_census`), and `radix_tree_dump` restates the builder, so that the depth is a
# prediction a CPU test pins.
LADDER_BITS = 10           # Morton bits per axis (k_keys: 1024 cells along every axis)
CORNER_EXTENT = 32.0
CORNER_CELL = CORNER_EXTENT / 1024.0
CORNER_MAIN = dict(log2_soup=10, seed=61)    # 1 056 triangles: radix tree 41 deep, up to 40 frames pending
CORNER_SECOND = dict(log2_soup=15, seed=62)  # 32 800 triangles: 46 deep, up to 45 pending
CORNER_DEPTH = {10: 41, 15: 46}              # 30 Morton bits, the corner pin against the soup, log2_soup index bits
CORNER_WIDE = dict(log2_soup=13, seed=62)    # 8 224 triangles: the HOST-collapsed 8-wide tree is 19 levels deep (CORNER_SECOND's: 22)
CORNER_WIDE_DEPTH = {13: 19, 15: 22}         # levels of bvh_wide_build_host's tree (tests/test_wide_census.py pins them)


def corner_ladder_scene(sg, log2_soup, seed, extent=CORNER_EXTENT):
    """A scene whose radix tree is 31 + log2_soup deep, with cell = extent / 1024 (one Morton cell when the far pin bounds the scene):
      * a ladder of 30 triangles, one per Morton bit b = 0..9 and axis a = 0..2: centroid c with c[a] = 1.1 * 2^b cells and 0.4 * 2^b cells on
        the other two axes, vertices 0, 1.5 c + w and 1.5 c - w with w uniform in +-0.5 c per component. The highest set bit of the
        centroid's Morton code is bit b of axis a, and the triangle's box has the corner (0, 0, 0) as its minimum;
      * two pins of 1e-3 cell, at the corner and at (extent, extent, extent);
      * a soup of 2^log2_soup triangles with vertices uniform in [0.02, 0.98]^3 cells: one Morton cell, split by leaf-index bits alone.
    (A ladder vertex of bit 9 may reach 1.1 * extent: the cells then shrink by up to 1 / 1.1, which keeps every centroid's highest bit.) Every
    coordinate is 0 or within the exact fast-division range [2^-37, 2^40] of the traversal. The camera sits at 0.5 cell (1, 1, 1) and looks
    along (1, 1, 1). Material 0 is plain, material 1 emits: the ladder's first triangle (bit 0, axis 0: it crosses the soup's cell) and every
    4th soup triangle. The ladder triangle alone leaves every render black, whichever of the 30 it is: no ladder triangle comes nearer than
    0.4 cell to the camera, and a path in the soup moves 0.005 cell per bounce (the oracle, 48x32x2: no pixel above 0, no ray of the
    replayed paths reaches the emitter), so an image could not tell a wrong hit from a right one. Triangle order: soup, corner pin, far pin, ladder (bit-major): the run of equal codes is then leaves 0 .. 2^log2_soup (the
    corner pin last), which the leaf-index bits halve log2_soup times."""
    rng = np.random.default_rng(seed)
    cell = extent / 1024.0
    ladder = np.zeros((3 * LADDER_BITS, 3, 3))
    for b in range(LADDER_BITS):
        for a in range(3):
            c = np.full(3, 0.4 * 2.0 ** b)
            c[a] = 1.1 * 2.0 ** b
            w = rng.uniform(-0.5, 0.5, size=3) * c
            ladder[3 * b + a, 1], ladder[3 * b + a, 2] = 1.5 * c + w, 1.5 * c - w
    e = 1e-3
    pins = np.array([[[0, 0, 0], [e, 0, 0], [0, e, 0]], [[1024, 1024, 1024], [1024 - e, 1024, 1024], [1024, 1024 - e, 1024]]], dtype=np.float64)
    soup = rng.uniform(0.02, 0.98, size=(2 ** log2_soup, 3, 3))
    pos = (np.concatenate([soup, pins, ladder]) * cell).astype(np.float32)
    n = len(pos)
    nz = np.abs(pos[pos != 0])
    assert (pos >= 0).all() and nz.min() >= 2.0 ** -37 and nz.max() <= 2.0 ** 40
    tan = np.zeros((n, 3, 3), dtype=np.float32)
    tan[..., 0] = 1.0
    ids = np.zeros(n, dtype=np.uint32)
    ids[len(soup) + len(pins)] = 1
    ids[0 : len(soup) : 4] = 1
    mats = [sg.Material(color=(0.8, 0.8, 0.8, 1.0), roughness=1.0, metallic=0.0),
            sg.Material(color=(1.0, 1.0, 1.0, 1.0), emission=(1.0, 0.9, 0.8), emissive_strength=2.0, roughness=1.0, metallic=0.0)]
    f32 = lambda v: (np.asarray(v, dtype=np.float64) / np.linalg.norm(v)).astype(np.float32)  # noqa: E731
    fwd, right = f32([1, 1, 1]), f32([-1, 0, 1])  # right = forward x (0, 1, 0), up = right x forward, as scenegen.look_camera's basis
    cam = sg.Camera(position=np.full(3, 0.5 * cell, dtype=np.float32), right=right, up=f32(np.cross([-1, 0, 1], [1, 1, 1])), forward=fwd,
                    fov_x=sg.look_camera((0, 0, 0)).fov_x)
    return sg.Scene(positions=pos, normals=None, texcoords=np.zeros((n, 3, 2), dtype=np.float32), tangents=tan, material_ids=ids, materials=mats,
                    textures=[], camera=cam)


def corner_rays(cell, n, seed):
    """Rays that start inside every box on the path to the soup of a corner_ladder_scene: origins uniform in [0.3, 0.7]^3 cells, directions
    in the positive octant (components uniform in [0.3, 1] before normalising: at least 0.2 after)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(0.3, 0.7, size=(n, 3)) * cell
    d = rng.uniform(0.3, 1.0, size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], axis=1).astype(np.float32)


def octant_rays(cell, n, seed):
    """corner_rays(cell, n, seed) with the direction of ray k turned into octant k % 8: bit a of k % 8 set = component a negative (the
    octant numbering of csrc/rt_wide.hip wide_init). The 8-wide walk takes a node's slots in the order slot ^ octant, so every octant
    is another visiting order of the same tree; the origins stay inside the soup."""
    rays = corner_rays(cell, n, seed)
    k = np.arange(n) % 8
    for a in range(3):
        rays[:, 3 + a] = np.where((k >> a) & 1, -rays[:, 3 + a], rays[:, 3 + a])
    return rays


def _spread10(v):
    v = v.astype(np.uint32) & np.uint32(1023)
    for shift, mask in ((16, 0x030000FF), (8, 0x0300F00F), (4, 0x030C30C3), (2, 0x09249249)):
        v = (v | (v << np.uint32(shift))) & np.uint32(mask)
    return v


def morton_keys(positions):
    """k_keys of csrc/rt_bvh_device.hip in float32: the 30-bit Morton code of every triangle's centre, (p0 + p1 + p2) / 3, on the 1024^3 grid of
    the bounds of all vertices (x in bits 0, 3, ..., y one above, z two above)."""
    p = np.ascontiguousarray(positions, dtype=np.float32)
    lo, hi = p.reshape(-1, 3).min(axis=0), p.reshape(-1, 3).max(axis=0)
    ext = hi - lo
    with np.errstate(divide="ignore"):
        inv = np.where(ext > 0, np.float32(1024.0) / ext, np.float32(0.0)).astype(np.float32)
    ctr = ((p[:, 0] + p[:, 1]) + p[:, 2]) / np.float32(3.0)
    q = np.minimum(np.maximum((ctr - lo) * inv, np.float32(0.0)), np.float32(1023.0)).astype(np.uint32)
    return _spread10(q[:, 0]) | (_spread10(q[:, 1]) << np.uint32(1)) | (_spread10(q[:, 2]) << np.uint32(2))


def radix_tree_dump(positions):
    """The tree RT_BUILDER_LBVH builds of `positions` (one triangle per leaf), restated in numpy and returned as a bvh_device_dump record set
    {root, nodes, tris} plus "order" (the leaf order) and "keys" (the Morton codes, in triangle order):
      * the leaves are the triangles in the stable order of their Morton codes (radix_sort_pairs); leaf k has the 64-bit key code << 32 | k;
      * Karras 2012: the node over leaves [lo, hi] splits after the last leaf that shares with leaf lo more leading key bits than leaf hi does;
        an inner child takes the index of the end of its range that touches the split (left: its last leaf, right: its first), the root is 0;
      * every stored child box is the box of the vertices below (k_refit)."""
    pos = np.ascontiguousarray(positions, dtype=np.float32)
    n = len(pos)
    codes = morton_keys(pos)
    order = np.argsort(codes, kind="stable").astype(np.uint32)
    keys = (codes[order].astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    p = pos[order]
    tris = np.zeros((n, 12), dtype=np.uint32)
    tris[:, 0:3] = p[:, 0].view(np.uint32)
    tris[:, 3:6] = (p[:, 1] - p[:, 0]).astype(np.float32).view(np.uint32)
    tris[:, 6:9] = (p[:, 2] - p[:, 0]).astype(np.float32).view(np.uint32)
    tris[:, 9] = order
    tris[:, 10] = 3  # first and last triangle of its leaf
    out = {"order": order, "keys": codes, "tris": tris, "nodes": np.zeros((max(n - 1, 0), 16), dtype=np.uint32)}
    if n <= 1:
        out["root"] = (LEAF | (1 << 27)) if n else NONE
        return out
    tlo, thi = p.min(axis=1), p.max(axis=1)
    nodes = out["nodes"]
    boxes = nodes[:, :12].view(np.float32)
    todo = [(0, 0, n - 1)]
    while todo:
        i, lo, hi = todo.pop()
        top = int(keys[lo] ^ keys[hi]).bit_length() - 1  # the highest bit in which the range's keys differ
        first_set = ((int(keys[lo]) >> top) | 1) << top  # the smallest key with lo's prefix and that bit set
        g = int(np.searchsorted(keys, np.uint64(first_set), side="left")) - 1
        assert lo <= g < hi
        for side, (a, b, idx) in enumerate(((lo, g, g), (g + 1, hi, g + 1))):
            boxes[i, 6 * side : 6 * side + 3] = tlo[a : b + 1].min(axis=0)
            boxes[i, 6 * side + 3 : 6 * side + 6] = thi[a : b + 1].max(axis=0)
            if a == b:
                nodes[i, 12 + side] = LEAF | (1 << 27) | a
            else:
                nodes[i, 12 + side] = idx
                todo.append((idx, a, b))
    out["root"] = 0
    return out


def dump_depth(dump):
    """Edges on the longest path from the root of a bvh_device_dump record set to a leaf."""
    if dump["root"] == NONE or dump["root"] & LEAF:
        return 0
    refs = dump["nodes"][:, 12:14]
    level, depth = np.array([dump["root"]], dtype=np.uint32), 0
    while len(level):
        depth += 1
        kids = refs[level].reshape(-1)
        level = kids[(kids & LEAF) == 0]
    return depth


def _first_max(v):  # *std::max_element over the last axis: the FIRST largest, by operator<
    m = v[..., 0]
    for k in (1, 2):
        m = np.where(m < v[..., k], v[..., k], m)
    return m


def _first_min(v):
    m = v[..., 0]
    for k in (1, 2):
        m = np.where(v[..., k] < m, v[..., k], m)
    return m


def _det(c1, c2, c3):  # dot(c1, crs(c2, c3)) with the reference's operation order, float32
    x = c2[:, 1] * c3[:, 2] - c2[:, 2] * c3[:, 1]
    y = c2[:, 2] * c3[:, 0] - c2[:, 0] * c3[:, 2]
    z = c2[:, 0] * c3[:, 1] - c2[:, 1] * c3[:, 0]
    return c1[:, 0] * x + c1[:, 1] * y + c1[:, 2] * z


def dump_census(dump, rays):
    """OracleScene.walk_census's closest-hit count for the tree the DEVICE built: per ray, the largest number of deferred siblings pending at
    once when the reference's traversal rule (oracle/rt_oracle.cpp BVH::intersect_ray, which every binary closest-hit kernel follows) walks a
    bvh_device_dump record set. The oracle's own box and triangle tests walk the records (oracle.dump_census); `dump_census_numpy` states the
    rule a second time, and tests/test_walk_census.py holds both to walk_census on flattened reference trees."""
    import oracle

    return oracle.dump_census(dump, rays).astype(np.int64)


def dump_census_numpy(dump, rays, eps=1e-4, max_stack=256):
    """dump_census restated in numpy (slow: for a few thousand rays on small trees). OracleScene.walk_census's closest-hit count for a tree given as a bvh_device_dump record set (child boxes in words 0..11 of a node record,
    child references in words 12 and 13, triangles as a, b - a, c - a): for every ray the largest number of deferred siblings pending at once
    under the reference's traversal rule (oracle/rt_oracle.cpp BVH::intersect_ray), which every binary closest-hit kernel follows:
      * a child is hit when t_min <= t_max and t_max >= eps of the float32 slabs (intersect_box), its distance is d = max(t_min, eps);
      * both children hit: the left one is walked first unless d_left > d_right, and the other is deferred (one more pending);
      * when the near subtree is done the deferred child is entered, unless the near subtree found a hit with t <= its d (pruned).
    All of it in float32 with the reference's operation order (min / max and the first-largest rule of std::max_element included), so the counts
    ARE walk_census's when the dump is the flattened reference tree (tests/test_walk_census.py). All rays walk in lockstep, one node or one
    triangle per step."""
    nodes, tris, root = dump["nodes"], dump["tris"], int(dump["root"])
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = len(rays)
    most = np.zeros(n, dtype=np.int64)
    if root == NONE or n == 0:
        return most
    eps = np.float32(eps)
    boxes = np.ascontiguousarray(nodes[:, :12]).view(np.float32).reshape(-1, 2, 2, 3)  # [node, child, lo / hi, axis]
    refs = np.ascontiguousarray(nodes[:, 12:14])
    tf = np.ascontiguousarray(tris[:, :9]).view(np.float32)
    ta, tv, tu = tf[:, 0:3], tf[:, 3:6], tf[:, 6:9]
    last = (tris[:, 10] & 1) != 0
    # per ray, by original index: the stack of deferred children, and best[r, k] = the closest hit found since k frames were pending
    sp = np.zeros(n, dtype=np.int64)
    st_ref = np.zeros((n, max_stack), dtype=np.uint32)
    st_d = np.zeros((n, max_stack), dtype=np.float32)
    best = np.full((n, max_stack + 1), np.inf, dtype=np.float32)
    # the rays still walking (compacted): original index, origin, direction, current reference
    idx = np.arange(n)
    o, d = rays[:, :3].copy(), rays[:, 3:].copy()
    cur = np.full(n, root, dtype=np.uint32)
    with np.errstate(all="ignore"):
        while len(idx):
            is_leaf = (cur & LEAF) != 0
            pop = np.zeros(len(idx), dtype=bool)
            L = np.flatnonzero(is_leaf)
            if len(L):  # one triangle of the leaf: the reference's intersect_tri
                ref = cur[L]
                k = (ref & MASK).astype(np.int64)
                cnt = (ref >> 27) & 15
                av, au, at, y = tv[k], tu[k], -d[L], o[L] - ta[k]
                den = _det(av, au, at)
                xb, xc, xt = _det(y, au, at) / den, _det(av, y, at) / den, _det(av, au, y) / den
                hit = (xb >= 0) & (xc >= 0) & (xb + xc <= 1) & (xt >= eps)
                r = idx[L[hit]]
                best[r, sp[r]] = np.minimum(best[r, sp[r]], xt[hit])
                done = np.where(cnt > 0, cnt == 1, last[k])
                cur[L] = np.where(cnt > 0, LEAF | ((cnt - 1) << 27) | (k + 1).astype(np.uint32), LEAF | (k + 1).astype(np.uint32)).astype(np.uint32)
                pop[L[done]] = True
            I = np.flatnonzero(~is_leaf)
            if len(I):  # an inner node: the reference's intersect_box on both children
                nd = cur[I]
                b = boxes[nd]
                i12 = (b - o[I][:, None, None, :]) / d[I][:, None, None, :]
                i1, i2 = i12[:, :, 0], i12[:, :, 1]
                t_min = _first_max(np.where(i2 < i1, i2, i1))  # std::min(a, b) = b < a ? b : a
                t_max = _first_min(np.where(i1 < i2, i2, i1))  # std::max(a, b) = a < b ? b : a
                hit = (t_min <= t_max) & (t_max >= eps)
                dist = np.where(t_min < eps, eps, t_min)
                kid = refs[nd]
                both = hit[:, 0] & hit[:, 1]
                right_first = (both & (dist[:, 0] > dist[:, 1])) | (~hit[:, 0] & hit[:, 1])
                near = np.where(right_first, kid[:, 1], kid[:, 0])
                cur[I] = near
                pop[I[~hit[:, 0] & ~hit[:, 1]]] = True
                B = np.flatnonzero(both)
                if len(B):
                    r = idx[I[B]]
                    s = sp[r]
                    assert s.max() < max_stack, "dump_census_numpy: more frames pending than max_stack"
                    st_ref[r, s] = np.where(right_first[B], kid[B, 0], kid[B, 1])
                    st_d[r, s] = np.where(right_first[B], dist[B, 0], dist[B, 1])
                    best[r, s + 1] = np.inf
                    sp[r] = s + 1
                    most[r] = np.maximum(most[r], s + 1)
            P = np.flatnonzero(pop)
            finished = np.zeros(len(idx), dtype=bool)
            while len(P):  # the subtree is done: enter the newest deferred child, or prune it and look at the next
                r = idx[P]
                s = sp[r]
                finished[P[s == 0]] = True
                P, r, s = P[s > 0], r[s > 0], s[s > 0]
                found = best[r, s]
                sp[r] = s - 1
                best[r, s - 1] = np.minimum(best[r, s - 1], found)
                enter = ~(found <= st_d[r, s - 1])  # bvh.h: if (!intr.has || intr.t > d_right)
                cur[P[enter]] = st_ref[r[enter], s[enter] - 1]
                P = P[~enter]
            if finished.any():
                keep = ~finished
                idx, o, d, cur = idx[keep], o[keep], d[keep], cur[keep]
    return most


# ------------------------------------------------------------------------------------------------ the census of the 8-wide walk
# A radix tree 41 deep does not make the 8-wide walk deep: a wide level absorbs about three binary levels, and the siblings along the radix
# chain are single triangles, which the collapse keeps as LEAF slots of the chain's nodes, tested on the spot and never stacked (CORNER_MAIN:
# 144 wide nodes on 10 levels, 5 groups pending at most). What keeps groups pending is a node with several INNER slots whose boxes all hold the
# ray, level after level: the HOST-collapsed tree of the soup (bvh_wide_build_host over the reference's SAH tree) is 19 levels deep for 2^13
# soup triangles and 22 for 2^15, and rays from inside the soup keep 12 to 19 groups pending in every direction octant.
def wide_tree_order(tree):
    """order[k] = the scene triangle of triangle record k: a host tree's "order", or word 9 of a dump's triangle records."""
    return np.ascontiguousarray(tree["order"] if "order" in tree else tree["tris"][:, 9], dtype=np.uint32)


def wide_census(tree, positions, rays):
    """Per ray, the largest number of node groups pending at once when the rule of the 8-wide closest-hit kernel (csrc/rt_wide.hip
    wide_node_step and the unwind of wf_extend_wide) walks the 80-byte WideNode records of `tree`: bvh_wide_build_host's result or
    DeviceScene.bvh_wide_dump's, with `positions` the scene's triangles. The rule:
      * the root is a pseudo-group of one slot; a group is {first inner child, pending priority bits, inner-slot mask};
      * a step takes the highest pending priority bit; a slot's priority is slot ^ oct_inv, oct_inv = 7 ^ the direction-sign octant;
      * the step pushes the rest of the group as ONE frame if any inner slot remains pending: one more group pending, however many slots;
      * it then tests the child's eight boxes against [EPS, best.t]; the hit inner slots become the current group;
      * the triangles of the hit leaf slots are tested before the next step (a closer t replaces best.t);
      * a group with nothing pending pops the newest frame, which is not tested again against the best.t found since.
    Boxes are tested in float64 on the de-quantised planes, p + q * 2^(e - 127), by (plane - o) * (1 / d), with 1 / d = +-2^60 for a
    component below 2^-60 as in the kernel; an empty slot is never hit. Triangles are tested by the oracle's own test.
    A pending count g means g - 1 groups behind the one in registers: the 10th (WIDE_RING_EVICT) evicts from the 8-deep LDS ring.
    The DEVICE does not test these boxes: its planes are the same bytes, but the slab test is float32 FMAs with an explicit margin, so it
    may enter a box this walk does not (never the reverse) and its count may differ by a box at one level or two. The tests therefore never
    claim the eviction threshold itself: every claim is "share of rays at >= 12" (WIDE_CLAIM), two groups past the first eviction, so that
    a walk which differs from this one by a group or two still evicts and refills.
    The walk itself is the oracle's (oracle.wide_census, C++); `wide_census_numpy` states it a second time."""
    import oracle

    return oracle.wide_census(tree["nodes"], wide_tree_order(tree), positions, rays).astype(np.int64)


def wide_tree_arrays(tree):
    """The fields of (n, 20) uint32 WideNode records the walk reads: de-quantised lower and upper planes [node, axis, slot] in float64,
    inner-slot mask, child_base, tri_base, tri_mask."""
    nodes = np.ascontiguousarray(tree["nodes"], dtype=np.uint32).reshape(-1, 20)
    b = nodes.view(np.uint8).reshape(-1, 80)
    p = np.ascontiguousarray(nodes[:, 0:3]).view(np.float32).astype(np.float64)
    cell = np.ldexp(1.0, b[:, 12:15].astype(np.int32) - 127)
    lo = p[:, :, None] + b[:, 32:56].reshape(-1, 3, 8).astype(np.float64) * cell[:, :, None]
    hi = p[:, :, None] + b[:, 56:80].reshape(-1, 3, 8).astype(np.float64) * cell[:, :, None]
    return lo, hi, b[:, 15].astype(np.int64), nodes[:, 4].astype(np.int64), nodes[:, 5].astype(np.int64), nodes[:, 6].astype(np.int64)


def wide_census_numpy(tree, positions, rays, eps=1e-4):
    """wide_census restated in Python, one ray at a time (for a few hundred rays). Same rule, same arithmetic: float64 boxes, float32
    triangle tests in the reference's operation order (`_det`), so the counts equal the C++ census ray for ray (tests/test_wide_census.py).
    What does not depend on the walk is computed for the whole tree at once per ray (every slot's entry and exit parameter, every triangle
    record's t); the walk then only compares them with the best t it has."""
    lo, hi, imask, child_base, tri_base, tri_mask = wide_tree_arrays(tree)
    order = wide_tree_order(tree).astype(np.int64)
    tri = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3, 3)[order]  # in record order
    ta, tv, tu = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    eps32 = np.float32(eps)
    most = np.zeros(len(rays), dtype=np.int64)
    if len(lo) == 0:
        return most
    popcount = lambda v: bin(v).count("1")  # noqa: E731
    imask, child_base, tri_base, tri_mask = imask.tolist(), child_base.tolist(), tri_base.tolist(), tri_mask.tolist()
    for r, ray in enumerate(rays):
        o32, d32 = ray[:3], ray[3:]
        o, d = o32.astype(np.float64), d32.astype(np.float64)
        with np.errstate(divide="ignore"):
            idir = np.where(np.abs(d) < 2.0 ** -60, np.copysign(2.0 ** 60, d), 1.0 / d)
        neg = idir < 0
        oct_inv = 7 ^ int(neg[0] + 2 * neg[1] + 4 * neg[2])
        t0, t1 = (lo - o[None, :, None]) * idir[None, :, None], (hi - o[None, :, None]) * idir[None, :, None]
        enter = np.maximum(np.where(neg[None, :, None], t1, t0).max(axis=1), float(eps32)).tolist()  # [node][slot]
        leave = np.where(neg[None, :, None], t0, t1).min(axis=1).tolist()
        with np.errstate(all="ignore"):  # the reference's intersect_tri on every triangle record, float32
            at, y = np.broadcast_to(-d32, tv.shape), o32 - ta
            den = _det(tv, tu, at)
            xb, xc, xt = _det(y, tu, at) / den, _det(tv, y, at) / den, _det(tv, tu, y) / den
            tri_t = np.where((xb >= 0) & (xc >= 0) & (xb + xc <= 1) & (xt >= eps32), xt, np.float32(np.inf)).astype(np.float64).tolist()
        best = float("inf")
        stack = []
        base, bits, inner = 0, 0x80, 0  # the root: one pending slot of a group whose children start at record 0
        while True:
            if bits == 0:
                if not stack:
                    break
                base, bits, inner = stack.pop()
                continue
            bit = bits.bit_length() - 1
            rest, slot = bits ^ (1 << bit), bit ^ oct_inv
            i = base + popcount(inner & ((1 << slot) - 1))
            if rest:
                stack.append((base, rest, inner))
                most[r] = max(most[r], len(stack))
            base, bits, inner, tmask = child_base[i], 0, imask[i], tri_mask[i]
            limit = best  # all eight boxes are tested before any triangle of the node
            for s in range(8):
                is_inner, n_tri = inner >> s & 1, popcount((tmask >> (3 * s)) & 7)
                if not (is_inner or n_tri) or not enter[i][s] <= min(leave[i][s], limit):
                    continue
                if is_inner:
                    bits |= 1 << (s ^ oct_inv)
                else:
                    first = tri_base[i] + popcount(tmask & ((1 << (3 * s)) - 1))
                    best = min(best, min(tri_t[first : first + n_tri]))
    return most


