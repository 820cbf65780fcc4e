"""The BVH as it sits in HBM (rt_bvh_device_dump), for both builders:
  * reference-topology host build (default): the flattened DevNode / DevTri arrays the kernels read equal an independent
    flattening (in numpy) of the reference-style node list the CPU tests pin to the reference's BVH dumps;
  * device LBVH build (RT_BUILD_DEVICE_LBVH, csrc/rt_bvh_device.hip): a different topology, validated by
    invariants (every triangle in exactly one leaf, every stored child box is the exact bounding box of its subtree, bounded
    depth and leaf size) and by closest-hit equality against the CPU ORACLE (never another GPU scene): identical t, bit for
    bit, on 10^5 rays; an index may differ only on an exact tie, and the tie share is asserted against a number."""
import numpy as np
import pytest

import hit_contract
from bvh_dump import check_invariants, compare_hits_with_oracle, flatten_reference
from conftest import random_rays
from hit_contract import explain_pixels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report_hit_contract_time():
    t0 = hit_contract.STATS["seconds"]
    yield
    print(f"\n[hit contract] {hit_contract.STATS['seconds'] - t0:.1f} s of this module's run spent in verify_hits / explain_pixels")

@pytest.mark.parametrize("name", ["room_plain", "boxes", "room_manylights"])
def test_device_memory_holds_the_reference_topology(gpu, scenes, name):
    sc = scenes[name]
    dev = gpu.DeviceScene(sc)
    try:
        for which in (0, 1):
            info, dump = dev.bvh_info(which), dev.bvh_device_dump(which)
            nodes, tris, root = flatten_reference(info, sc.positions)
            assert dump["root"] == root
            assert np.array_equal(dump["nodes"][:, :14], nodes[:, :14]), which
            assert np.array_equal(dump["tris"][:, :11], tris[:, :11]), which
    finally:
        dev.close()


@pytest.mark.parametrize("case", ["room_5000", "boxes", "tiny_1", "tiny_2", "tiny_5", "tiny_9", "room_1M", "room_5000/lbvh", "boxes/lbvh", "tiny_9/lbvh", "room_1M/lbvh"])
def test_device_lbvh_invariants_and_closest_hits(gpu, oracle, sg, case, monkeypatch):
    """Both binary builders of rt_bvh_device.hip: PLOC (default; agglomerative clustering along the Morton order) and the Karras
    radix tree + refit (rt_build_options.device_builder = RT_BUILDER_LBVH, also PLOC's fallback for trees deeper than the traversal stacks)."""
    case, _, builder = case.partition("/")
    opts = {"device_builder": gpu.RT_BUILDER_LBVH} if builder == "lbvh" else {}
    if case.startswith("room"):
        n = 5000 if case == "room_5000" else 1_000_000
        sc = sg.room_scene(n, seed=3, n_lights=6, n_materials=8, tex_size=8, n_tex_sets=2, offset=0.15 if n == 5000 else 0.05)
    elif case == "boxes":
        sc = sg.boxes_scene(n_boxes=40, seed=4, n_lights=3)
    else:
        k = int(case.split("_")[1])
        rng = np.random.default_rng(k)
        pos = rng.uniform(-2, 2, size=(k, 3, 3)).astype(np.float32)
        tan = np.tile(np.array([1, 0, 0], dtype=np.float32), (k, 3, 1))
        sc = sg.Scene(positions=pos, normals=None, texcoords=np.zeros((k, 3, 2), np.float32), tangents=tan, material_ids=np.zeros(k, np.uint32),
                      materials=[sg.Material(color=(0.7, 0.7, 0.7, 1.0), roughness=1.0, metallic=0.0)], textures=[],
                      camera=sg.look_camera((0.0, 0.0, 6.0), yaw_deg=0.0, yfov=0.9))
    orc = oracle.OracleScene(sc)
    dev = gpu.DeviceScene(sc, device_bvh=True, **opts)
    try:
        dump = dev.bvh_device_dump(0)
        depth = check_invariants(dump, sc.positions, max_leaf=4)
        info = dev.bvh_info(0)  # reference-style description rebuilt from HBM
        leaves = info["nodes"][info["nodes"][:, 6] == 0xFFFFFFFF]
        assert (leaves[:, 9] - leaves[:, 8]).sum() == sc.n_triangles and sorted(info["order"].tolist()) == list(range(sc.n_triangles))
        n_rays = 100_000 if sc.n_triangles >= 5000 else 20_000
        rays = random_rays(sc, n_rays, seed=12)
        # random triangle soups do not tie; the boxes scene does along the shared diagonal of a face's two triangles
        ties = compare_hits_with_oracle(orc, dev, rays, max_tie_share=2e-3 if case == "boxes" else 5e-5, brute="all" if sc.n_triangles <= 50_000 else 256)
        # the render loop runs unchanged on the device-built tree: both schedules agree, and the image is the ORACLE's wherever
        # no path met an exact tie
        W, H, SPP = (96, 64, 4) if sc.n_triangles >= 5000 else (48, 32, 4)
        a, _ = orc.run_raytracer(W, H, SPP, seed=5)
        b, _ = dev.run_raytracer(W, H, SPP, seed=5)
        m, _ = dev.run_raytracer(W, H, SPP, seed=5, megakernel=True)
        assert np.isfinite(b).all() and np.array_equal(b.view(np.uint32), m.view(np.uint32))
        rel = np.abs(a - b) / np.maximum(np.abs(a), 1e-6)
        differing = float((rel > 1e-5).any(axis=2).mean())
        assert differing <= (0.02 if case == "boxes" else 0.002), differing  # only paths through an exact tie can differ
        # ... which every pixel that differs in ANY bit shows: the first differing hit of one of its paths is a tie, verified bit for bit
        bits = (a.view(np.uint32) != b.view(np.uint32)).any(axis=2)
        recs = explain_pixels(orc, dev, W, H, SPP, 5, np.argwhere(bits), "exact", packet=False, brute="all" if sc.n_triangles <= 50_000 else 0, what=case)
        assert all(r["cause"] == "exact tie" for r in recs), recs
        t_dev = dev.build_times()
        print(f"\\n[{case}] {builder or 'ploc'}: triangles {sc.n_triangles}: device build {t_dev['build_ms']:.2f} ms (+ upload {t_dev['upload_ms']:.1f} ms), depth {depth}, "
              f"tie share vs oracle {ties:.2e}, pixels beyond 1e-5 of the oracle {differing:.2e}")
    finally:
        orc.close()
        dev.close()


def test_ploc_terminates_on_collapsed_geometry(gpu, oracle, sg):
    """Found by tools/soak_wide_rays.py: 20 000 triangles of a needle-shaped soup 4096 extents away from the origin, where float32 leaves the y and z
    coordinates one or two distinct values. Every cluster union then has the same (zero) surface area; PLOC's nearest-neighbour search, which used to
    resolve ties to the lowest position, merged ONE pair per round and gave up after 4096 rounds (RT_ERR_HIP "PLOC did not terminate"). Now the pairing
    partner wins ties and a round that merges less than 1/32 of the clusters is followed by a forced pairing round: the build finishes, the tree is a
    proper BVH over all triangles, and its closest hits are the oracle's up to the coordinates' own resolution (hit / miss equal; the wide tree: nothing lost, nothing farther)."""
    rng = np.random.default_rng(56)
    n, scale = 20_000, float(2 ** 17)
    shape = np.array([1.0, 1e-4, 1e-4])
    offset = np.array([-0.6, 0.8, -0.7]) * 4096 * scale
    c = rng.uniform(-1.0, 1.0, size=(n, 1, 3)) * shape
    pos = ((c + rng.uniform(-1.0, 1.0, size=(n, 3, 3)) * 0.1 * shape) * scale + offset).astype(np.float32)
    assert len(np.unique(pos[..., 1])) <= 4 and len(np.unique(pos[..., 2])) <= 4  # the collapse this test is about
    tang = np.tile(np.array([1, 0, 0], dtype=np.float32), (n, 3, 1))
    sc = sg.Scene(positions=pos, normals=None, texcoords=np.zeros((n, 3, 2), np.float32), tangents=tang, material_ids=np.zeros(n, np.uint32),
                  materials=[sg.Material(color=(0.7, 0.7, 0.7, 1.0), roughness=1.0, metallic=0.0)], textures=[],
                  camera=sg.look_camera(tuple(float(v) for v in offset + np.array([0.0, 0.0, 3.0 * scale])), yaw_deg=0.0, yfov=0.9))
    rays = random_rays(sc, 20_000, seed=3)
    orc = oracle.OracleScene(sc)
    try:
        op, ob = orc.cast_rays(rays)
        for kw in (dict(device_bvh=True), dict(device_bvh=True, wide=True)):
            dev = gpu.DeviceScene(sc, **kw)  # raised RT_ERR_HIP before the fix
            try:
                if not kw.get("wide"):
                    depth = check_invariants(dev.bvh_device_dump(0), sc.positions, max_leaf=4)
                    assert depth <= 62
                gp, gb, _ = dev.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
                if kw.get("wide"):  # the superset contract: nothing lost, nothing farther
                    assert not ((gp == 0xFFFFFFFF) & (op != 0xFFFFFFFF)).any()
                    both = (gp != 0xFFFFFFFF) & (op != 0xFFFFFFFF)
                    assert (gb[both, 2] <= ob[both, 2]).all()
                else:
                    assert np.array_equal(gp == 0xFFFFFFFF, op == 0xFFFFFFFF)
                    both = op != 0xFFFFFFFF
                    # which of several coincident candidates the reference's pruning rule finds depends on the tree; their computed distances differ by
                    # what the COORDINATES resolve here (ulp of 3e8 = 32, against extents of 26 in y and z), not by an ulp of t
                    tol = 8.0 * float(np.spacing(np.float32(np.abs(pos).max())))
                    assert np.abs(gb[both, 2].astype(np.float64) - ob[both, 2].astype(np.float64)).max(initial=0.0) <= tol
            finally:
                dev.close()
    finally:
        orc.close()

