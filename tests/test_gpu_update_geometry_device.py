"""GPU tests of rt_update_geometry_device (include/rt_abi.h): rt_update_geometry for arrays that are in HBM already.

The host-array path is the specification, bit for bit: scene A is updated with update_geometry(new), scene B with
update_geometry_device(torch tensors of geometry_arrays(new)) — the same bytes — and every output and dump of the two must be equal as bytes
(after two host-path scenes have been shown to agree). Nothing is compared with a tolerance. 64x48x4 renders of the fixture scenes (400-600
triangles) unless a test says otherwise.

One thing two scenes of the HOST path do not agree on: the numbering of the records of a tree that was built on the device. PLOC and the
device collapse hand out node and triangle-record indices with atomicAdd, so two builds of the same arrays give the same tree under different
indices (the renders, casts and counters agree; tests/test_gpu_update_geometry.py therefore never compares such dumps between scenes).
Dumps of device-built trees are compared here in canonical form: the records in pre-order from the root, children in slot order, with the
index words (a binary node's references to inner children, a wide node's child_base and tri_base, the record index in DevTri::pad) left out
and every other word kept. Trees built on the
host, the light tree included, are compared as raw bytes."""
import dataclasses

import numpy as np
import pytest

from deep_walks import light_query_rays, volume_lights_scene
from test_gpu_update_geometry import COUNTERS, KINDS, SEED, SPP, WIDE_KINDS, H, W, assert_same, bits, outputs, same_dump
from update_geometry import POINT_ON_GRID, TINY_SIZES, deform, relight

pytestmark = pytest.mark.gpu

NAMES = ["room_manylights", "room_textured", "boxes"]
MODES = [("rebuild", k) for k in sorted(KINDS)] + [("refit", k) for k in sorted(WIDE_KINDS)]


def kind_kw(mode, kind):
    return KINDS[kind] if mode == "rebuild" else WIDE_KINDS[kind]


def on_gpu(gpu, new, shift=0):
    """geometry_arrays(new) as torch tensors on GPU 0. shift > 0: each is a view that starts `shift` elements into a larger storage."""
    import torch

    arrays = new if isinstance(new, dict) else gpu.geometry_arrays(new)
    out = {}
    for k, a in arrays.items():
        a = a.view(np.int32) if a.dtype == np.uint32 else a
        t = torch.zeros(a.size + shift, dtype=torch.int32 if a.dtype == np.int32 else torch.float32, device="cuda:0")
        t[shift:] = torch.from_numpy(a)
        out[k] = t[shift:]
    torch.cuda.synchronize()
    return out


def canon_binary(d):
    """A device-built binary tree (bvh_device_dump(0)) in pre-order. A DevNode is 16 words: the two child boxes (12), left, right, pad[2].
    Kept per node: the boxes, each reference to a LEAF child (leaves lie in Morton order, which is a function of the arrays), and the two pad
    words; a reference to an inner child is an index the build handed out and is replaced by 0, the child follows in pre-order. The triangle
    records as they are."""
    nodes, out = d["nodes"], []
    stack = [d["root"]] if len(nodes) else []
    while stack:
        ref = stack.pop()
        if ref & 0x80000000:
            continue
        row = nodes[ref]
        leaf = [int(r) if int(r) & 0x80000000 else 0 for r in row[12:14]]
        out.append(np.concatenate([row[:12], leaf, row[14:16]]).astype(np.uint32))
        stack += [int(row[13]), int(row[12])]
    assert len(out) == len(nodes), "the walk must reach every node"
    return {"depth": d["root"] if d["root"] & 0x80000000 else 0, "nodes": np.array(out, dtype=np.uint32).reshape(-1, 16), "tris": d["tris"]}


def canon_wide(d):
    """An 8-wide tree (bvh_wide_dump) in pre-order: per node every word but child_base and tri_base (words 4, 5), then its triangle records
    without the record index (word 11), then its inner children in slot order."""
    nodes, tris, rows, trows = d["nodes"], d["tris"], [], []
    stack = [0] if len(nodes) else []
    while stack:
        row = nodes[stack.pop()]
        rows.append(np.concatenate([row[:4], row[6:]]))
        n_tri, n_inner = bin(int(row[6])).count("1"), bin(int(row[3]) >> 24).count("1")
        trows.extend(tris[int(row[5]) + j, :11] for j in range(n_tri))
        stack += [int(row[4]) + r for r in reversed(range(n_inner))]
    assert len(rows) == len(nodes) and len(trows) == len(tris), "the walk must reach every record"
    return {"depth": d["depth"], "nodes": np.array(rows, dtype=np.uint32).reshape(-1, 18), "tris": np.array(trows, dtype=np.uint32).reshape(-1, 11)}


def scene_tree(dev, kw):
    """The scene tree as the kernels see it, comparable between two scenes (the module docstring says why device-built ones are canonicalised)."""
    d = dev.bvh_wide_dump() if kw.get("wide") else dev.bvh_device_dump(0)
    if not kw.get("device_bvh"):
        return d
    return canon_wide(d) if kw.get("wide") else canon_binary(d)


def same_tree(a, b, kw):
    return same_dump(scene_tree(a, kw), scene_tree(b, kw))


def dumps(dev, kw, info0=True):
    """The trees as arrays: the light tree as the kernels and as the host see it, the scene tree as the kernels see it (and, on the reference
    build, as the host does)."""
    out = {}
    for which, d in ((1, dev.bvh_device_dump(1)), (0, scene_tree(dev, kw))):
        out[f"dump{which}.head"] = np.array([d.get("root", d.get("depth"))], dtype=np.uint32)
        out[f"dump{which}.nodes"], out[f"dump{which}.tris"] = d["nodes"], d["tris"]
    for which in (0, 1) if (not kw and info0) else (1,):
        i = dev.bvh_info(which)
        out[f"info{which}.root"], out[f"info{which}.nodes"], out[f"info{which}.order"] = np.array([i["root"]], dtype=np.uint32), i["nodes"], i["order"]
    return out


def everything(gpu, dev, sc, kw):
    return {**outputs(gpu, dev, sc, kw), **dumps(dev, kw)}


# ------------------------------------------------------------------------------------------------------------ 1. equals the host path
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode, kind", MODES)
def test_device_update_equals_the_host_path(gpu, scenes, mode, kind, name):
    kw, refit = kind_kw(mode, kind), mode == "refit"
    sc = scenes[name]
    steps = [("wave", deform(sc, "wave")), ("relight", relight(sc)), ("back to the creation arrays", sc)]
    a1, a2, b = (gpu.DeviceScene(sc, **kw) for _ in range(3))
    try:
        for what, new in steps:
            a1.update_geometry(new, refit=refit)
            a2.update_geometry(new, refit=refit)
            want = everything(gpu, a1, new, kw)
            assert_same(want, everything(gpu, a2, new, kw), f"{mode}, {kind}, {name}, {what}: two host-path scenes")
            b.update_geometry_device(**on_gpu(gpu, new), refit=refit)
            assert_same(everything(gpu, b, new, kw), want, f"{mode}, {kind}, {name}, {what}: device arrays against host arrays")
            if refit:  # the binary tree the wide one was collapsed from no longer describes either scene
                for dev in (a1, b):
                    with pytest.raises(gpu.RtError) as e:
                        dev.bvh_info(0)
                    assert e.value.code == 8
            bt_a, bt_b = a1.build_times(), b.build_times()
            assert (bt_b["wide_ms"] > 0) == (bt_a["wide_ms"] > 0) == bool(kw.get("wide")) and bt_b["build_ms"] >= 0
            if not refit and kw.get("device_bvh"):
                assert bt_b["upload_ms"] == 0 and bt_a["upload_ms"] > 0  # nothing was uploaded: the build read the caller's arrays
        # the packet policy was reset with each update: the next render measures it again, and agrees
        fa, sa = a1.run_raytracer(W, H, SPP, seed=SEED, counters=True)
        fb, sb = b.run_raytracer(W, H, SPP, seed=SEED, counters=True)
        assert np.array_equal(bits(fa), bits(fb)) and [sa[k] for k in COUNTERS] == [sb[k] for k in COUNTERS]
    finally:
        for d in (a1, a2, b):
            d.close()


# ------------------------------------------------------------------------------------------------------------ 2. light order across blocks
def test_lights_of_many_blocks_keep_their_order(gpu, sg):
    """912 triangles with 600 lights scattered over all of them by one fixed permutation: each of the compaction's four 256-triangle chunks holds
    some, and the light list must still reach the host builder in ascending triangle order — the light tree is the host path's, bit for bit."""
    base = volume_lights_scene(sg, n_lights=600, size=3.0, seed=5)
    perm = np.random.default_rng(77).permutation(base.n_triangles)
    sc = dataclasses.replace(base, positions=base.positions[perm], normals=None, texcoords=base.texcoords[perm], tangents=base.tangents[perm],
                             material_ids=np.asarray(base.material_ids, dtype=np.uint32)[perm])
    em = np.array([bool((m.emission_f32() != 0).any()) for m in sc.materials])
    lights = np.flatnonzero(em[sc.material_ids])
    assert len(lights) == 600 and len(np.unique(lights // 256)) >= 3, "the test needs lights in at least three 256-triangle blocks"
    assert sc.n_triangles > 3 * 256
    rays = light_query_rays(sc, 4096, seed=3)
    kw = KINDS["device_wide"]
    dark = relight(sc, off=True)
    assert not em[dark.material_ids].any()
    for refit in (True, False):
        a, b = gpu.DeviceScene(sc, **kw), gpu.DeviceScene(sc, **kw)
        try:
            for what, new in (("wave", deform(sc, "wave")), ("no light at all", dark), ("back", sc)):
                a.update_geometry(new, refit=refit)
                b.update_geometry_device(**on_gpu(gpu, new), refit=refit)
                ia, ib = a.bvh_info(1), b.bvh_info(1)
                assert ia["root"] == ib["root"] and ia["nodes"].tobytes() == ib["nodes"].tobytes() and ia["order"].tobytes() == ib["order"].tobytes(), (refit, what)
                da, db = a.bvh_device_dump(1), b.bvh_device_dump(1)
                assert da["root"] == db["root"] and da["nodes"].tobytes() == db["nodes"].tobytes() and da["tris"].tobytes() == db["tris"].tobytes(), (refit, what)
                assert len(ia["order"]) == (0 if new is dark else 600)
                assert np.array_equal(bits(a.light_pdf(rays)), bits(b.light_pdf(rays))), (refit, what)
                assert same_tree(a, b, kw), (refit, what)
            assert np.array_equal(bits(a.run_raytracer(W, H, SPP, seed=SEED)[0]), bits(b.run_raytracer(W, H, SPP, seed=SEED)[0]))
        finally:
            a.close()
            b.close()


def test_more_chunks_than_the_scan_has_blocks(gpu, scenes):
    """The scan and the compaction launch at most 4096 blocks and stride over the 256-triangle chunks beyond: 4096 * 256 + 777 triangles put
    lights, a bad id and non-finite floats into chunks only a second trip of the loop reaches. Light tree, light pdf, casts and render
    against the host path, both modes (the scene trees of a million triangles are not walked in Python here: the casts go through them)."""
    base = scenes["room_plain"]
    n = 4096 * 256 + 777
    rng = np.random.default_rng(2024)
    cen = rng.uniform(-10, 10, size=(n, 1, 3))
    pos = (cen + rng.uniform(-0.05, 0.05, size=(n, 3, 3))).astype(np.float32)
    em = np.array([bool((m.emission_f32() != 0).any()) for m in base.materials])
    plain, light = int(np.flatnonzero(~em)[0]), int(np.flatnonzero(em)[0])
    ids = np.full(n, plain, dtype=np.uint32)
    lights = np.unique(np.concatenate([rng.integers(0, n, size=400), [3, 4096 * 256 - 1, 4096 * 256, 4096 * 256 + 5, n - 1]]))
    ids[lights] = light
    assert (lights >= 4096 * 256).sum() >= 3 and (lights < 256).any()
    tan = np.zeros((n, 3, 3), dtype=np.float32)
    tan[..., 0] = 1.0
    sc = dataclasses.replace(base, positions=pos, normals=None, texcoords=np.zeros((n, 3, 2), dtype=np.float32), tangents=tan, material_ids=ids)
    new = relight(deform(sc, "wave"))  # other positions and another light set, again with lights in the last chunks
    new_lights = np.flatnonzero(em[new.material_ids])
    assert len(new_lights) and not np.array_equal(new_lights, lights)
    ids2 = np.asarray(new.material_ids, dtype=np.uint32).copy()
    ids2[[4096 * 256 + 9, n - 2]] = light
    new = dataclasses.replace(new, material_ids=ids2)
    # 2048 rays from inside the cloud, half of them aimed at light centroids (deep_walks.light_query_rays loops over all triangles in Python)
    org = rng.uniform(-10, 10, size=(2048, 3))
    tgt = new.positions[np.flatnonzero(em[new.material_ids])].mean(axis=1)
    d = np.where(np.arange(2048)[:, None] < 1024, tgt[rng.integers(0, len(tgt), size=2048)] - org, rng.normal(size=(2048, 3)))
    rays = np.concatenate([org, d / np.linalg.norm(d, axis=1, keepdims=True)], axis=1).astype(np.float32)
    kw = KINDS["device_wide"]
    a, b = gpu.DeviceScene(sc, **kw), gpu.DeviceScene(sc, **kw)
    try:
        arrays = gpu.geometry_arrays(new)
        for refit in (True, False):
            a.update_geometry(new, refit=refit)
            b.update_geometry_device(**on_gpu(gpu, arrays), refit=refit)
            ia, ib = a.bvh_info(1), b.bvh_info(1)
            assert ia["root"] == ib["root"] and ia["nodes"].tobytes() == ib["nodes"].tobytes() and ia["order"].tobytes() == ib["order"].tobytes(), refit
            assert np.array_equal(np.sort(ib["order"]), np.flatnonzero(em[new.material_ids])), refit
            da, db = a.bvh_device_dump(1), b.bvh_device_dump(1)
            assert da["root"] == db["root"] and da["nodes"].tobytes() == db["nodes"].tobytes() and da["tris"].tobytes() == db["tris"].tobytes(), refit
            assert np.array_equal(bits(a.light_pdf(rays)), bits(b.light_pdf(rays))), refit
            pa, ba, _ = a.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
            pb, bb, _ = b.cast_rays_ex(rays, gpu.RT_CAST_EXTEND)
            assert np.array_equal(pa, pb) and np.array_equal(bits(ba), bits(bb)), refit
            assert np.array_equal(bits(a.run_raytracer(W, H, SPP, seed=SEED)[0]), bits(b.run_raytracer(W, H, SPP, seed=SEED)[0])), refit
        fb0 = bits(b.run_raytracer(W, H, SPP, seed=SEED)[0]).copy()
        for where, named in (([n - 3], n - 3), ([n - 3, 4096 * 256 + 2], 4096 * 256 + 2), ([n - 3, 4096 * 256 + 2, 7], 7)):
            bad = dict(arrays, positions=arrays["positions"].copy())
            bad["positions"].reshape(-1, 3, 3)[where, 2, 1] = np.nan
            with pytest.raises(gpu.RtError) as e:
                b.update_geometry_device(**on_gpu(gpu, bad), refit=True)
            assert e.value.code == 1 and f"(triangle {named})" in str(e.value), str(e.value)
        bad = dict(arrays, material_ids=arrays["material_ids"].copy())
        bad["material_ids"][n - 1] = len(base.materials)
        with pytest.raises(gpu.RtError) as e:
            b.update_geometry_device(**on_gpu(gpu, bad))
        assert e.value.code == 1 and "material id" in str(e.value)
        assert np.array_equal(bits(b.run_raytracer(W, H, SPP, seed=SEED)[0]), fb0), "a refused update changed the scene"
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------------------ 3. buffers
@pytest.mark.parametrize("mode, kind", MODES)
def test_arrays_are_read_only_not_retained_and_need_four_byte_alignment_only(gpu, scenes, mode, kind):
    import torch

    kw, refit = kind_kw(mode, kind), mode == "refit"
    sc = scenes["room_textured"]
    new = deform(sc, "wave")
    a, b = gpu.DeviceScene(sc, **kw), gpu.DeviceScene(sc, **kw)
    try:
        a.update_geometry(new, refit=refit)
        want = everything(gpu, a, new, kw)
        t = on_gpu(gpu, new, shift=1)  # one element into a larger storage: 4-byte aligned, not 8- or 16-byte aligned
        assert all(v.data_ptr() % 16 == 4 and v.storage_offset() == 1 for v in t.values())
        before = {k: v.cpu().numpy().tobytes() for k, v in t.items()}
        b.update_geometry_device(**t, refit=refit)
        assert all(v.cpu().numpy().tobytes() == before[k] for k, v in t.items()), "the call wrote to the caller's arrays"
        fb = b.run_raytracer(W, H, SPP, seed=SEED)[0]
        for k, v in t.items():  # the caller may overwrite them as soon as the call has returned
            v.fill_(float("nan") if v.dtype == torch.float32 else 0x7FFFFFFF)
        torch.cuda.synchronize()
        assert np.array_equal(bits(b.run_raytracer(W, H, SPP, seed=SEED)[0]), bits(fb)), "the scene still reads the caller's arrays"
        del t
        assert_same(everything(gpu, b, new, kw), want, f"{mode}, {kind}: misaligned views, overwritten after the call")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------------------ 4. tiny scenes
@pytest.mark.parametrize("kind", sorted(WIDE_KINDS))
def test_tiny_scenes(gpu, scenes, kind):
    """0 triangles, root-only trees, and both sides of the 8-triangle threshold under which a wide scene is collapsed on the host (there a
    device REBUILD stages its arrays; a REFIT never does)."""
    kw = WIDE_KINDS[kind]
    sc = scenes["room_plain"]
    for n in TINY_SIZES:
        tiny = dataclasses.replace(sc, positions=sc.positions[:n], normals=None, texcoords=sc.texcoords[:n], tangents=sc.tangents[:n], material_ids=sc.material_ids[:n])
        moved = relight(deform(tiny, "scatter", seed=n)) if n else tiny
        a, b = gpu.DeviceScene(tiny, **kw), gpu.DeviceScene(tiny, **kw)
        try:
            for what, new, refit in (("rebuild", moved, False), ("refit back", tiny, True), ("refit", moved, True), ("rebuild back", tiny, False)):
                a.update_geometry(new, refit=refit)
                b.update_geometry_device(**on_gpu(gpu, new), refit=refit)
                if n == 0:
                    continue
                assert same_tree(a, b, kw), (n, what)
                assert_same(dumps(b, kw), dumps(a, kw), f"{kind}, {n} triangles, {what}")
            assert np.array_equal(bits(a.run_raytracer(W, H, SPP, seed=SEED)[0]), bits(b.run_raytracer(W, H, SPP, seed=SEED)[0])), n
        finally:
            a.close()
            b.close()


# ------------------------------------------------------------------------------------------------------------ 5. refusals
def state(dev, kw):
    d = dev.bvh_wide_dump() if kw.get("wide") else dev.bvh_device_dump(0)
    l = dev.bvh_device_dump(1)
    return (bits(dev.run_raytracer(W, H, SPP, seed=SEED)[0]).tobytes(), d["nodes"].tobytes(), d["tris"].tobytes(), l["nodes"].tobytes(), l["tris"].tobytes())


def refused(gpu, dev, kw, tensors, code, refit=False, **more):
    """The call is refused with `code`, and render and dumps are afterwards what they were, bit for bit. Returns the message."""
    before = state(dev, kw)
    with pytest.raises(gpu.RtError) as e:
        dev.update_geometry_device(**tensors, refit=refit, **more)
    assert e.value.code == code, str(e.value)
    assert state(dev, kw) == before, f"a refused update changed the scene: {e.value}"
    return str(e.value)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_refusals_leave_the_scene_unchanged(gpu, scenes, kind):
    import torch

    kw = KINDS[kind]
    sc = scenes["room_plain"]
    good = gpu.geometry_arrays(deform(sc, "wave"))
    dev = gpu.DeviceScene(sc, **kw)
    try:
        for refit in (False, True) if kw.get("wide") else (False,):
            bad = {k: v.copy() for k, v in good.items()}
            bad["positions"].reshape(-1, 3, 3)[17, 1, 2] = np.nan
            msg = refused(gpu, dev, kw, on_gpu(gpu, bad), 1, refit)
            assert "non-finite" in msg and "17" in msg
            bad["positions"].reshape(-1, 3, 3)[300, 0, 0] = np.nan  # a second one, in another block of the scan: the lowest is named
            msg = refused(gpu, dev, kw, on_gpu(gpu, bad), 1, refit)
            assert "non-finite" in msg and "(triangle 17)" in msg
            bad = {k: v.copy() for k, v in good.items()}
            bad["positions"].reshape(-1, 3, 3)[sc.n_triangles - 1, 2, 1] = np.inf
            msg = refused(gpu, dev, kw, on_gpu(gpu, bad), 1, refit)
            assert "non-finite" in msg and f"(triangle {sc.n_triangles - 1})" in msg
            bad = {k: v.copy() for k, v in good.items()}
            bad["material_ids"][5] = len(sc.materials)
            assert "material id" in refused(gpu, dev, kw, on_gpu(gpu, bad), 1, refit)
            bad["positions"].reshape(-1, 3, 3)[2, 0, 0] = np.nan  # both: the material id is the host path's first complaint
            assert "material id" in refused(gpu, dev, kw, on_gpu(gpu, bad), 1, refit)
            n = sc.n_triangles - 1
            per = {name: p for name, p, _ in gpu.GEOMETRY_ARRAYS}
            fewer = {k: v[: n * per[k]] for k, v in good.items()}
            assert "n_triangles" in refused(gpu, dev, kw, on_gpu(gpu, fewer), 1, refit)
            acc = dev.accumulator(W, H, seed=1)
            before = state(dev, kw)
            with pytest.raises(gpu.RtError) as e:
                dev.update_geometry_device(**on_gpu(gpu, good), refit=refit)
            assert e.value.code == 1 and "accumulator" in str(e.value)
            acc.close()
            assert state(dev, kw) == before
            # pinned host memory: a HIP pointer, but not device memory (and a check that missed it could not fault on it)
            t = on_gpu(gpu, good)
            pinned = torch.from_numpy(good["positions"]).pin_memory()
            assert pinned.is_pinned() and not pinned.is_cuda
            ptrs = {k: v.data_ptr() for k, v in t.items()}
            ptrs["positions"] = pinned.data_ptr()
            assert "not device memory" in refused(gpu, dev, kw, ptrs, 1, refit, n_triangles=sc.n_triangles)
        if not kw.get("wide"):
            assert "RT_BUILD_WIDE" in refused(gpu, dev, kw, on_gpu(gpu, good), 8, refit=True)
        else:
            for scale_log2 in (60, -70):
                far = dict(good, positions=(good["positions"] * np.float32(2.0) ** np.float32(scale_log2)).astype(np.float32))
                for refit in (False, True):
                    assert "exponent range" in refused(gpu, dev, kw, on_gpu(gpu, far), 8, refit)
            dot = dict(good, positions=np.ascontiguousarray(np.broadcast_to(POINT_ON_GRID, (sc.n_triangles * 3, 3)), dtype=np.float32).reshape(-1))
            for refit in (False, True):
                assert "exponent range" in refused(gpu, dev, kw, on_gpu(gpu, dot), 8, refit)
        # ... and a valid update still goes through, and is the host path's
        dev.update_geometry_device(**on_gpu(gpu, good))
        ref = gpu.DeviceScene(sc, **kw)
        try:
            ref.update_geometry(deform(sc, "wave"))
            assert_same({**outputs(gpu, dev, sc, kw), **dumps(dev, kw)}, {**outputs(gpu, ref, sc, kw), **dumps(ref, kw)}, f"{kind}: a valid update after the refusals")
        finally:
            ref.close()
    finally:
        dev.close()


def test_wrapper_checks_its_tensors(gpu, scenes):
    """DeviceScene.update_geometry_device refuses what it can see is wrong before the library is called."""
    import torch

    sc = scenes["room_plain"]
    dev = gpu.DeviceScene(sc, device_bvh=True, wide=True)
    try:
        t = on_gpu(gpu, sc)
        with pytest.raises(TypeError):
            dev.update_geometry_device(**dict(t, positions=t["positions"].double()))
        with pytest.raises(TypeError):
            dev.update_geometry_device(**dict(t, positions=t["positions"].cpu()))
        with pytest.raises(TypeError):
            dev.update_geometry_device(**dict(t, normals=None))
        with pytest.raises(TypeError):
            dev.update_geometry_device(**dict(t, material_ids=t["material_ids"].long()))
        with pytest.raises(ValueError):
            dev.update_geometry_device(**dict(t, texcoords=t["texcoords"][::2]))
        with pytest.raises(ValueError):
            dev.update_geometry_device(**dict(t, tangents=t["tangents"][:-9]))
        with pytest.raises(ValueError):
            dev.update_geometry_device(**{k: v.data_ptr() for k, v in t.items()})  # pointers alone do not say how many triangles
        before = state(dev, dict(wide=True))
        dev.update_geometry_device(**{k: v.data_ptr() for k, v in t.items()}, n_triangles=sc.n_triangles, refit=True)
        dev.update_geometry_device(**dict(t, material_ids=t["material_ids"].view(getattr(torch, "uint32", torch.int32))))
        assert state(dev, dict(wide=True)) == before
    finally:
        dev.close()


def test_multi_gpu_scenes_are_refused(gpu, scenes):
    sc = scenes["room_plain"]
    dev = gpu.DeviceScene(sc, device=[0, 0], build_flags=gpu.RT_BUILD_GROUP_COPY)
    try:
        t = on_gpu(gpu, deform(sc, "wave"))
        for refit in (False, True):
            fb0 = dev.run_raytracer(W, H, SPP, seed=SEED)[0]
            with pytest.raises(gpu.RtError) as e:
                dev.update_geometry_device(**t, refit=refit)
            assert e.value.code == 8 and "multi-GPU" in str(e.value)
            assert np.array_equal(bits(dev.run_raytracer(W, H, SPP, seed=SEED)[0]), bits(fb0))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------------------ 6. mixing entry points
@pytest.mark.parametrize("kind", sorted(WIDE_KINDS))
def test_entry_points_mix(gpu, scenes, kind):
    kw = WIDE_KINDS[kind]
    sc = scenes["room_manylights"]
    wave, scatter = deform(sc, "wave"), deform(sc, "scatter", seed=17)
    dev = gpu.DeviceScene(sc, **kw)
    try:
        dev.update_geometry_device(**on_gpu(gpu, wave), refit=True)
        dev.update_geometry(scatter)  # a host REBUILD: a new topology, of the scatter geometry
        rebuilt = dev.bvh_wide_dump()
        if kind == "host_collapsed":
            dev.bvh_info(0)  # a rebuilt scene answers again
        dev.update_geometry_device(**on_gpu(gpu, wave), refit=True)
        d = dev.bvh_wide_dump()
        model = gpu.bvh_wide_refit_host(rebuilt["nodes"], rebuilt["tris"][:, 9], wave.positions)
        assert d["nodes"].tobytes() == model.tobytes(), f"{int((d['nodes'] != model).any(axis=1).sum())} of {len(model)} nodes differ from rt_bvh_wide_refit_host"
        assert d["depth"] == rebuilt["depth"] and np.array_equal(d["tris"][:, 9:], rebuilt["tris"][:, 9:])
        acc = dev.accumulator(W, H, seed=SEED)
        acc.render(1)
        acc.render(SPP - 1)
        assert np.array_equal(bits(acc.image()), bits(dev.run_raytracer(W, H, SPP, seed=SEED)[0]))
        acc.close()
    finally:
        dev.close()


@pytest.mark.parametrize("kind", sorted(WIDE_KINDS))
def test_refit_times_report_the_last_refit(gpu, scenes, kind):
    """rt_refit_times: nothing before the first refit; afterwards the level pass is a part of the refit, through either entry point; a
    rebuild leaves the last refit's figures alone."""
    sc = scenes["room_manylights"]
    dev = gpu.DeviceScene(sc, **WIDE_KINDS[kind])
    try:
        assert dev.refit_times() == {"refit_ms": 0.0, "levels_ms": 0.0}
        for device_arrays in (True, False):
            new = deform(sc, "wave")
            dev.update_geometry_device(**on_gpu(gpu, new), refit=True) if device_arrays else dev.update_geometry(new, refit=True)
            t = dev.refit_times()
            assert 0 < t["levels_ms"] < t["refit_ms"], t
        dev.update_geometry_device(**on_gpu(gpu, sc))
        assert dev.refit_times() == t
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------------------ 7. no leak
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_device_updates_leak_no_device_memory(gpu, scenes, kind):
    """test_updates_leak_no_device_memory's 20 alternating updates and its bound, through the device entry point; both sets of arrays are on
    the GPU before the first update."""
    import torch

    kw = KINDS[kind]
    sc = scenes["room_manylights"]
    frames = [on_gpu(gpu, relight(deform(sc, "wave"))), on_gpu(gpu, sc)]
    dev = gpu.DeviceScene(sc, **kw)
    try:
        dev.run_raytracer(W, H, SPP, seed=SEED)
        free3 = None
        for i in range(20):
            dev.update_geometry_device(**frames[i % 2], refit=bool(kw.get("wide")) and i % 4 >= 2)
            if i == 2:
                free3 = torch.cuda.mem_get_info(0)[0]
        free20 = torch.cuda.mem_get_info(0)[0]
        print(f"{kind}: free after update 3: {free3}, after update 20: {free20}, one copy of the triangle records: {48 * sc.n_triangles}")
        assert abs(free20 - free3) < 48 * sc.n_triangles
    finally:
        dev.close()
