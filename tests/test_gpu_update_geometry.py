"""GPU tests of rt_update_geometry (include/rt_abi.h): new per-triangle arrays for a built scene.

RT_UPDATE_REBUILD must leave the scene rt_create would build from the new arrays: every output is compared bit for bit with a fresh
DeviceScene of the new geometry with the same flags (after two fresh scenes have been shown to agree on it), and on the reference build with
the oracle. RT_UPDATE_REFIT keeps the wide tree's topology: the dump must equal the CPU model (rt_bvh_wide_refit_host) applied to the previous
dump byte for byte, pass the exact containment walk of test_wide_build, and the traversal must keep the wide tree's hit contract
(hit_contract.verify_hits, kind "superset") against an oracle of the new geometry. Every refusal leaves the scene's render bit-equal.
The five fixture scenes (400-600 triangles), 64x48x4 renders."""
import dataclasses

import numpy as np
import pytest

from conftest import random_rays
from hit_contract import explain_pixels, verify_hits
from test_gpu_production import _camera_rays, compare_superset_hits_with_oracle
from test_wide_build import walk_and_check
from update_geometry import DEFORMATIONS, POINT_ON_GRID, TINY_SIZES, deform, relight, topology, tri_records

pytestmark = pytest.mark.gpu

FIXTURES = ["room_plain", "room_textured", "open_nolight", "boxes", "room_manylights"]
KINDS = {"reference": dict(), "reference_wide": dict(wide=True), "device": dict(device_bvh=True), "device_wide": dict(device_bvh=True, wide=True)}
WIDE_KINDS = {"host_collapsed": dict(wide=True), "device_collapsed": dict(device_bvh=True, wide=True)}
W, H, SPP, SEED = 64, 48, 4, 9
COUNTERS = ["samples", "casts", "nodes_visited", "box_tests", "tri_tests", "shaded_hits", "light_queries", "light_nodes", "light_box_tests",
            "light_tri_tests", "light_hits", "texel_fetches"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if np.asarray(a).dtype == np.float32 else np.asarray(a)


def probe_rays(sc, n_random, n_camera, seed):
    return np.concatenate([random_rays(sc, n_random, seed=seed), _camera_rays(sc, n_camera, seed=seed + 1)]).astype(np.float32)


def outputs(gpu, dev, sc, kw):
    """Everything an entry point returns for scene `sc` on `dev`, as name -> array (compared as bit patterns)."""
    out = {}
    fb, st = dev.run_raytracer(W, H, SPP, seed=SEED, counters=True)
    out["render"] = fb
    out["counters"] = np.array([st[k] for k in COUNTERS], dtype=np.uint64)
    rays = probe_rays(sc, 4096, 37, seed=31)
    for mode in (gpu.RT_CAST_PROBE, gpu.RT_CAST_EXTEND, gpu.RT_CAST_EXTEND_GLOBAL, gpu.RT_CAST_PACKET, gpu.RT_CAST_PACKET_GLOBAL):
        p, b, _ = dev.cast_rays_ex(rays, mode)
        out[f"cast{mode}.prim"], out[f"cast{mode}.bct"] = p, b
    out["light_pdf"] = dev.light_pdf(rays)
    if not kw.get("wide"):  # rt_surface_normals is a probe of the binary tree
        p, t, n, sn = dev.surface_normals(rays)
        out.update({"sn.prim": p, "sn.t": t, "sn.normal": n, "sn.shading": sn})
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs ({int((bits(a[k]) != bits(b[k])).sum())} words)"


def fresh_outputs(gpu, sc, kw):
    """Outputs of a fresh scene; two fresh scenes must agree on them, or the comparison with an updated scene means nothing."""
    outs = []
    for _ in range(2):
        d = gpu.DeviceScene(sc, **kw)
        try:
            outs.append(outputs(gpu, d, sc, kw))
        finally:
            d.close()
    assert_same(outs[0], outs[1], "two fresh scenes")
    return outs[0]


# ------------------------------------------------------------------------------------------------------------------------ REBUILD
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_rebuild_is_the_fresh_scene(gpu, oracle, scenes, kind, name):
    kw = KINDS[kind]
    sc = scenes[name]
    wave, relit = deform(sc, "wave"), relight(sc)
    dev = gpu.DeviceScene(sc, **kw)
    try:
        out_a = outputs(gpu, dev, sc, kw)
        for what, new in (("wave", wave), ("relight", relit)):
            dev.update_geometry(new)
            assert_same(outputs(gpu, dev, new, kw), fresh_outputs(gpu, new, kw), f"{kind}, {name}, {what}")
            fresh = gpu.DeviceScene(new, **kw)
            try:
                if kind == "reference":  # a parity scene stays a parity scene
                    orc = oracle.OracleScene(new)
                    ofb, ost = orc.run_raytracer(W, H, SPP, seed=SEED)
                    gfb, gst = dev.run_raytracer(W, H, SPP, seed=SEED, counters=True)
                    assert np.array_equal(bits(gfb), bits(ofb)), f"{name}, {what}: the updated parity scene's image is not the oracle's"
                    assert gst["casts"] == ost["casts"] and gst["nodes_visited"] == ost["nodes_visited"]
                    orc.close()
                    for extra in (dict(megakernel=True), dict(rng_mode=gpu.RT_RNG_REFERENCE)):
                        assert np.array_equal(bits(dev.run_raytracer(W, H, SPP, seed=SEED, **extra)[0]), bits(fresh.run_raytracer(W, H, SPP, seed=SEED, **extra)[0])), extra
                    for which in (0, 1):
                        a, b = dev.bvh_info(which), fresh.bvh_info(which)
                        assert a["root"] == b["root"] and np.array_equal(a["nodes"], b["nodes"]) and np.array_equal(a["order"], b["order"])
                        a, b = dev.bvh_device_dump(which), fresh.bvh_device_dump(which)
                        assert a["root"] == b["root"] and np.array_equal(a["nodes"], b["nodes"]) and np.array_equal(a["tris"], b["tris"])
                if kind == "reference_wide":
                    a, b = dev.bvh_wide_dump(), fresh.bvh_wide_dump()
                    assert a["depth"] == b["depth"] and np.array_equal(a["nodes"], b["nodes"]) and np.array_equal(a["tris"], b["tris"])
                bt = dev.build_times()
                assert bt["build_ms"] >= 0 and (bt["wide_ms"] > 0) == bool(kw.get("wide"))
            finally:
                fresh.close()
        # an accumulator created after an update is one of the new geometry
        acc = dev.accumulator(W, H, seed=SEED)
        acc.render(1)
        acc.render(SPP - 1)
        assert np.array_equal(bits(acc.image()), bits(dev.run_raytracer(W, H, SPP, seed=SEED)[0]))
        acc.close()
        dev.update_geometry(sc)  # A -> B -> A
        assert_same(outputs(gpu, dev, sc, kw), out_a, f"{kind}, {name}: back to the creation arrays")
    finally:
        dev.close()


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_updates_leak_no_device_memory(gpu, scenes, kind):
    """20 alternating updates: free device memory stays where it was after the third, to within one copy of the triangle records (a leaked
    buffer per update would be at least 17 of them)."""
    import torch

    kw = KINDS[kind]
    sc = scenes["room_manylights"]
    other = relight(deform(sc, "wave"))
    dev = gpu.DeviceScene(sc, **kw)
    try:
        dev.run_raytracer(W, H, SPP, seed=SEED)
        free3 = None
        for i in range(20):
            new = other if i % 2 == 0 else sc
            dev.update_geometry(new, refit=bool(kw.get("wide")) and i % 4 >= 2)
            if i == 2:
                free3 = torch.cuda.mem_get_info(0)[0]
        free20 = torch.cuda.mem_get_info(0)[0]
        print(f"{kind}: free after update 3: {free3}, after update 20: {free20}, one copy of the triangle records: {48 * sc.n_triangles}")
        assert abs(free20 - free3) < 48 * sc.n_triangles
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------------------------------ REFIT
def same_dump(a, b):
    return a["depth"] == b["depth"] and a["nodes"].tobytes() == b["nodes"].tobytes() and a["tris"].tobytes() == b["tris"].tobytes()


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("kind", sorted(WIDE_KINDS))
def test_refit_to_the_creation_arrays_is_the_identity(gpu, scenes, kind, name):
    dev = gpu.DeviceScene(scenes[name], **WIDE_KINDS[kind])
    try:
        before = dev.bvh_wide_dump()
        fb0 = dev.run_raytracer(W, H, SPP, seed=SEED)[0]
        dev.update_geometry(scenes[name], refit=True)
        assert same_dump(before, dev.bvh_wide_dump())
        assert np.array_equal(bits(dev.run_raytracer(W, H, SPP, seed=SEED)[0]), bits(fb0))
    finally:
        dev.close()


@pytest.mark.parametrize("kind", sorted(WIDE_KINDS))
def test_refit_of_tiny_scenes(gpu, oracle, scenes, kind):
    """Root-only trees and the sizes around the device collapse's threshold (scenes of <= 8 triangles are collapsed on the host)."""
    sc = scenes["room_plain"]
    for n in TINY_SIZES:
        tiny = dataclasses.replace(sc, positions=sc.positions[:n], normals=None, texcoords=sc.texcoords[:n], tangents=sc.tangents[:n], material_ids=sc.material_ids[:n])
        dev = gpu.DeviceScene(tiny, **WIDE_KINDS[kind])
        try:
            if n == 0:
                dev.update_geometry(tiny, refit=True)
                continue
            before = dev.bvh_wide_dump()
            dev.update_geometry(tiny, refit=True)
            assert same_dump(before, dev.bvh_wide_dump()), n
            moved = deform(tiny, "scatter", seed=n)
            dev.update_geometry(moved, refit=True)
            d = dev.bvh_wide_dump()
            order = d["tris"][:, 9]
            assert d["nodes"].tobytes() == gpu.bvh_wide_refit_host(before["nodes"], order, moved.positions).tobytes(), n
            walk_and_check(d["nodes"], order, moved.positions)
            rays = probe_rays(moved, 2000, 200, seed=n)
            orc = oracle.OracleScene(moved)
            op, ob = orc.cast_rays(rays)
            gp, gb, _ = dev.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
            verify_hits(orc, rays, op, ob, gp, gb, "superset", what=f"tiny scene of {n}, refitted")
            orc.close()
        finally:
            dev.close()


def first_hit_features(dev):
    acc = dev.accumulator(W, H, seed=SEED, features=True)
    try:
        acc.render(1)
        return acc.read_features()
    finally:
        acc.close()


@pytest.mark.parametrize("deformation", DEFORMATIONS)
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("kind", sorted(WIDE_KINDS))
def test_refit_follows_the_new_geometry(gpu, oracle, scenes, kind, name, deformation):
    kw = WIDE_KINDS[kind]
    sc = scenes[name]
    new = deform(sc, deformation, seed=17)
    dev = gpu.DeviceScene(sc, **kw)
    orc = oracle.OracleScene(new)
    try:
        before = dev.bvh_wide_dump()
        dev.update_geometry(new, refit=True)
        d = dev.bvh_wide_dump()
        order = before["tris"][:, 9]
        # the device refit is the CPU model, byte for byte: nodes and triangle records
        model = gpu.bvh_wide_refit_host(before["nodes"], order, new.positions)
        assert d["nodes"].tobytes() == model.tobytes(), f"{int((d['nodes'] != model).any(axis=1).sum())} of {len(model)} nodes differ from rt_bvh_wide_refit_host"
        assert d["depth"] == before["depth"] and np.array_equal(topology(d["nodes"]), topology(before["nodes"]))
        assert np.array_equal(d["tris"][:, 9:], before["tris"][:, 9:]), "prim, flags and record index of every triangle record stay"
        assert np.array_equal(d["tris"][:, :9], tri_records(new.positions, order)), "triangle records are (a, b - a, c - a) of the new positions"
        walk_and_check(d["nodes"], order, new.positions)
        # the hit contract of the wide tree, exactly, through the per-lane and the packet kernel
        rays = probe_rays(new, 20000, 8192, seed=201)
        op, ob = orc.cast_rays(rays)
        counts = {}
        for mode, what in ((gpu.RT_CAST_EXTEND, "per-lane"), (gpu.RT_CAST_PACKET, "packet")):
            gp, gb, _ = dev.cast_rays_ex(rays, mode)
            if deformation == "wave":
                counts[what] = compare_superset_hits_with_oracle(orc, rays, op, ob, gp, gb, f"{name}, {kind}, refit to {deformation}, {what}")
            else:
                verify_hits(orc, rays, op, ob, gp, gb, "superset", what=f"{name}, {kind}, refit to {deformation}, {what}")
        # lights and shading records against fresh scenes of the new geometry
        fresh = gpu.DeviceScene(new, **kw)
        parity = gpu.DeviceScene(new)
        try:
            assert np.array_equal(bits(dev.light_pdf(rays)), bits(fresh.light_pdf(rays)))
            # rt_surface_normals probes binary trees only; the first-hit features of an accumulator (albedo: material and uvs; shading normal:
            # normals, tangents, the normal map; depth: t) read the same shading records through the scene's own traversal. Equal to a fresh
            # parity scene's wherever the hit distance agrees; any other pixel must hold a legal tie or closer hit
            f, g = first_hit_features(dev), first_hit_features(parity)
            differ = np.zeros((H, W), dtype=bool)
            for k in f:
                x = bits(f[k]) != bits(g[k])
                differ |= x.any(axis=2) if x.ndim == 3 else x
            explain_pixels(orc, dev, W, H, 1, SEED, np.argwhere(differ), "superset", what=f"{name}, {kind}, refit to {deformation}: first-hit features")
            if deformation == "wave":
                cap = len(rays) // 500 + (40 if name == "boxes" else 0)  # test_wide_hits_equal_the_oracle's
                fp, fbct, _ = fresh.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
                fties, fcloser = compare_superset_hits_with_oracle(orc, rays, op, ob, fp, fbct, f"{name}, {kind}, fresh wide scene of the wave")
                assert fties + fcloser <= cap, (fties, fcloser)
                for what, (ties, closer) in counts.items():
                    print(f"{name}, {kind}, refit to wave, {what}: {ties} ties, {closer} closer hits (fresh tree: {fties}, {fcloser}; cap {cap})")
                    assert ties + closer <= cap, (what, ties, closer)
                gfb = dev.run_raytracer(W, H, SPP, seed=SEED)[0]
                ofb = orc.run_raytracer(W, H, SPP, seed=SEED)[0]
                explain_pixels(orc, dev, W, H, SPP, SEED, np.argwhere((bits(gfb) != bits(ofb)).any(axis=2)), "superset", what=f"{name}, {kind}, refit to wave: render")
        finally:
            fresh.close()
            parity.close()
        if deformation == "scatter":  # ... and back: the original bytes
            dev.update_geometry(sc, refit=True)
            assert same_dump(before, dev.bvh_wide_dump())
    finally:
        orc.close()
        dev.close()


@pytest.mark.parametrize("name", ["room_plain", "room_manylights", "boxes"])
@pytest.mark.parametrize("kind", sorted(WIDE_KINDS))
def test_refit_relights(gpu, scenes, kind, name):
    """Only material_ids change: the tree's bytes stay, the light set and the shading records follow. The tree is then the fresh scene's tree,
    so the whole render is the fresh scene's. room_plain: all lights off, and back."""
    kw = WIDE_KINDS[kind]
    sc = scenes[name]
    dev = gpu.DeviceScene(sc, **kw)
    try:
        before = dev.bvh_wide_dump()
        out0 = outputs(gpu, dev, sc, kw)
        steps = [relight(sc, off=True), sc] if name == "room_plain" else [relight(sc), sc]
        for new in steps:
            dev.update_geometry(new, refit=True)
            assert same_dump(before, dev.bvh_wide_dump())
            if new is sc:
                assert_same(outputs(gpu, dev, sc, kw), out0, f"{name}, {kind}: lights back")
            else:
                assert_same(outputs(gpu, dev, new, kw), fresh_outputs(gpu, new, kw), f"{name}, {kind}: relit by a refit")
                assert not np.array_equal(bits(outputs(gpu, dev, new, kw)["light_pdf"]), bits(out0["light_pdf"]))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------------------------------ refusals
def refused(gpu, dev, new, code, refit=False):
    fb0 = dev.run_raytracer(W, H, SPP, seed=SEED)[0]
    with pytest.raises(gpu.RtError) as e:
        dev.update_geometry(new, refit=refit)
    assert e.value.code == code, str(e.value)
    assert np.array_equal(bits(dev.run_raytracer(W, H, SPP, seed=SEED)[0]), bits(fb0)), "a refused update changed the scene"
    return str(e.value)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_refusals_leave_the_scene_unchanged(gpu, scenes, kind):
    kw = KINDS[kind]
    sc = scenes["room_plain"]
    dev = gpu.DeviceScene(sc, **kw)
    try:
        dump0 = dev.bvh_wide_dump() if kw.get("wide") else dev.bvh_device_dump(0)
        modes = (False, True) if kw.get("wide") else (False,)
        for refit in modes:
            pos = sc.positions.copy()
            pos[17, 1, 2] = np.nan
            assert "non-finite" in refused(gpu, dev, dataclasses.replace(sc, positions=pos), 1, refit)
            pos[17, 1, 2] = np.inf
            refused(gpu, dev, dataclasses.replace(sc, positions=pos), 1, refit)
            n = sc.n_triangles - 1
            fewer = dataclasses.replace(sc, positions=sc.positions[:n], normals=None, texcoords=sc.texcoords[:n], tangents=sc.tangents[:n], material_ids=sc.material_ids[:n])
            assert "n_triangles" in refused(gpu, dev, fewer, 1, refit)
            ids = np.asarray(sc.material_ids, dtype=np.uint32).copy()
            ids[5] = len(sc.materials)
            assert "material id" in refused(gpu, dev, dataclasses.replace(sc, material_ids=ids), 1, refit)
            acc = dev.accumulator(W, H, seed=1)
            assert "accumulator" in refused(gpu, dev, deform(sc, "wave"), 1, refit)
            acc.close()
        if not kw.get("wide"):
            assert "RT_BUILD_WIDE" in refused(gpu, dev, deform(sc, "wave"), 8, refit=True)
        else:  # scaled out of the wide tree's exponent range, as test_wide_build_refuses_scenes_outside_its_exponent_range scales
            for scale_log2 in (60, -70):
                k = np.float32(2.0) ** np.float32(scale_log2)
                far = dataclasses.replace(sc, positions=(sc.positions * k).astype(np.float32))
                for refit in (False, True):
                    assert "exponent range" in refused(gpu, dev, far, 8, refit)
            # no extent at all (every vertex at one point of the origin grid): rt_create's test refuses that too
            dot = dataclasses.replace(sc, positions=np.broadcast_to(POINT_ON_GRID, sc.positions.shape).astype(np.float32))
            with pytest.raises(gpu.RtError) as e:
                gpu.DeviceScene(dot, **kw)
            assert e.value.code == 8
            for refit in (False, True):
                assert "exponent range" in refused(gpu, dev, dot, 8, refit)
        dump1 = dev.bvh_wide_dump() if kw.get("wide") else dev.bvh_device_dump(0)
        assert dump0["nodes"].tobytes() == dump1["nodes"].tobytes() and dump0["tris"].tobytes() == dump1["tris"].tobytes()
        dev.update_geometry(deform(sc, "wave"))  # the accumulator is gone: now it goes through
    finally:
        dev.close()


def test_multi_gpu_scenes_are_refused(gpu, scenes):
    sc = scenes["room_plain"]
    dev = gpu.DeviceScene(sc, device=[0, 0], build_flags=gpu.RT_BUILD_GROUP_COPY)
    try:
        for refit in (False, True):
            assert "multi-GPU" in refused(gpu, dev, deform(sc, "wave"), 8, refit)
    finally:
        dev.close()
