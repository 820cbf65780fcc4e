"""Host and device destinations of every entry point that takes RT_FLAG_DEVICE_FB give the same bits (csrc/rt_call_io.h: the caller's pointer,
or a region of the call's one staging block that is copied back), at the smallest shapes at which a slipped offset or size shows: a 5 x 3 and
a 1 x 1 image, 7 rays, 3 bake points. A null destination leaves the other results alone; a sharded render touches only its own blocks of a host
destination. Everything compared here is a bit pattern; there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEVICE_FB = 1  # RT_FLAG_DEVICE_FB
SPP = 4


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def scene(sg):
    return sg.room_scene(800, seed=21, n_lights=4, n_materials=6, tex_size=16, n_tex_sets=2, alpha_fraction=0.2)


@pytest.fixture(scope="module")
def dev(gpu, scene):
    d = gpu.DeviceScene(scene)
    yield d
    d.close()


@pytest.fixture(scope="module")
def hbm(dev):
    """hbm(n_bytes) -> a uint8 torch tensor on the scene's device, prefilled with 0xA5 and idle"""
    import torch

    def make(n_bytes):
        t = torch.full((int(n_bytes),), 0xA5, dtype=torch.uint8, device=f"cuda:{dev._device}")
        torch.cuda.synchronize()
        return t

    return make


def _same(host, t):
    got = t.cpu().numpy()
    assert got.size == _bits(host).size and np.array_equal(got, _bits(host))


@pytest.mark.parametrize("w,h", [(5, 3), (1, 1)])
def test_images_host_and_device_destination_agree(gpu, dev, hbm, w, h):
    lib = gpu.lib()
    n = w * h
    fb, _ = dev.run_raytracer(w, h, SPP, seed=3)
    t = hbm(12 * n)
    dev.run_raytracer(w, h, SPP, seed=3, device_fb=t.data_ptr())
    assert np.isfinite(fb).all() and fb.max() > 0
    _same(fb, t)
    img, _ = dev.run_raytracer_rgb8(w, h, SPP, seed=3)
    t = hbm(3 * n)
    dev.run_raytracer_rgb8(w, h, SPP, seed=3, device_rgb8=t.data_ptr())
    _same(img, t)

    acc = dev.accumulator(w, h, seed=5, features=True, ids="primitive")
    acc.render(SPP)
    for host, call, nbytes in (
        (acc.image(), lambda p: lib.rt_accum_resolve(acc._h, DEVICE_FB, p), 12 * n),
        (acc.image(rgb8=True), lambda p: lib.rt_accum_resolve_rgb8(acc._h, DEVICE_FB, p), 3 * n),
        (acc.denoise(), lambda p: lib.rt_accum_denoise(acc._h, None, DEVICE_FB, p), 12 * n),
        (acc.denoise(rgb8=True), lambda p: lib.rt_accum_denoise_rgb8(acc._h, None, DEVICE_FB, p), 3 * n),
        (acc.matte([0, 1, 2, 3, 5, 8]), lambda p: acc.matte([0, 1, 2, 3, 5, 8], device_out=p.value) or 0, 4 * n),
    ):
        t = hbm(nbytes)
        assert call(C.c_void_p(t.data_ptr())) == 0
        _same(host, t)

    # three and two destinations of one call; each may be null, on the host and in HBM, and the others do not move
    feats = acc.features()
    full = [feats["albedo"], feats["normal"], feats["depth"]]
    assert any(a.any() for a in full)
    for skip in (None, 0, 1, 2):
        ts = [hbm(a.nbytes) for a in full]
        hs = [np.full_like(a, np.nan) for a in full]
        assert lib.rt_accum_resolve_features(acc._h, DEVICE_FB, *(C.c_void_p(t.data_ptr()) if k != skip else None for k, t in enumerate(ts))) == 0
        assert lib.rt_accum_resolve_features(acc._h, 0, *(_ptr(a) if k != skip else None for k, a in enumerate(hs))) == 0
        for k in range(3):
            if k == skip:
                assert bool((ts[k] == 0xA5).all()) and np.isnan(hs[k]).all()
            else:
                _same(full[k], ts[k])
                assert np.array_equal(_bits(hs[k]), _bits(full[k]))
    label, cov = acc.labels()
    assert cov.any()
    for skip in (None, 0, 1):
        ts = [hbm(4 * n), hbm(4 * n)]
        hs = [np.full((h, w), 0xA5A5A5A5, dtype=np.uint32), np.full((h, w), np.nan, dtype=np.float32)]
        before = [a.copy() for a in hs]
        acc.labels(device_out=[t.data_ptr() if k != skip else None for k, t in enumerate(ts)])
        assert lib.rt_accum_resolve_labels(acc._h, 0, *(_ptr(a) if k != skip else None for k, a in enumerate(hs))) == 0
        for k, want in enumerate((label, cov)):
            if k == skip:
                assert bool((ts[k] == 0xA5).all()) and np.array_equal(_bits(hs[k]), _bits(before[k]))
            else:
                _same(want, ts[k])
                assert np.array_equal(_bits(hs[k]), _bits(want))
    acc.close()


def test_rays_and_bakes_host_and_device_arrays_agree(gpu, dev, hbm, scene):
    import torch

    sensor = gpu.Sensor.pinhole(scene.camera, seed=9)
    rays = dev.sensor_rays(sensor, 7, 1, 1)  # 7 rays, one per output
    assert len(rays) == 7
    d_rays = hbm(7 * 32)
    dev.sensor_rays(sensor, 7, 1, 1, device_out=d_rays.data_ptr())
    _same(rays, d_rays)
    for rgb8 in (False, True):
        out, _ = dev.render_rays(rays, samples=SPP, seed=2, rgb8=rgb8)
        t = hbm(7 * (3 if rgb8 else 12))
        dev.render_rays(None, samples=SPP, seed=2, rgb8=rgb8, device_rays=d_rays.data_ptr(), n_rays=7, device_out=t.data_ptr())
        assert out.any()
        _same(out, t)

    # 3 bake points: the centroids of the scene's first three triangles, along their geometric normals
    tri = gpu.geometry_arrays(scene)["positions"].reshape(-1, 3, 3)[:3].astype(np.float64)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    pts = gpu.pack_bake_points(tri.mean(axis=1), nrm / np.linalg.norm(nrm, axis=1, keepdims=True), stream=[11, 5, 7])
    d_pts = torch.from_numpy(pts.view(np.uint8).copy()).to(d_rays.device)
    torch.cuda.synchronize()
    for bake, floats in ((dev.bake_irradiance, 3), (dev.bake_sh, 27)):
        out, _ = bake(pts, SPP, seed=4)
        t = hbm(3 * floats * 4)
        bake(None, SPP, seed=4, device_points=d_pts.data_ptr(), n_points=3, device_out=t.data_ptr())
        assert np.isfinite(out).all()
        _same(out, t)
    recs = dev.bake_rays(pts, SPP, seed=4)
    t = hbm(3 * SPP * 32)
    dev.bake_rays(None, SPP, seed=4, device_points=d_pts.data_ptr(), n_points=3, device_out=t.data_ptr())
    assert len(recs) == 3 * SPP
    _same(recs, t)

    # a 4 x 3 atlas of two triangles: a few texels, all four host arrays staged in one block
    P = np.array([[0, 0, 0, 1, 0, 0, 0, 0, 1], [2, 0, 0, 3, 0, 0, 2, 0, 1]], dtype=np.float32)
    N = np.tile(np.array([0, 1, 0], dtype=np.float32), (2, 3))
    uv = np.array([[0.0, 0.0, 0.6, 0.0, 0.0, 0.9], [0.5, 0.5, 1.0, 0.5, 1.0, 1.0]], dtype=np.float32)
    lm_pts, lm_tex = dev.lightmap_points(P, N, uv, 4, 3)
    assert 3 <= len(lm_tex) < 12
    dP, dN, dU = (torch.from_numpy(a).to(d_rays.device) for a in (P, N, uv))
    t_pts, t_tex = hbm(12 * 32), hbm(12 * 4)
    assert dev.lightmap_points(dP, dN, dU, 4, 3, device_points=t_pts.data_ptr(), device_texels=t_tex.data_ptr()) == len(lm_tex)
    k = len(lm_tex)
    _same(lm_pts, t_pts[: 32 * k])
    _same(lm_tex, t_tex[: 4 * k])
    assert bool((t_pts[32 * k:] == 0xA5).all()) and bool((t_tex[4 * k:] == 0xA5).all())


def test_a_sharded_render_touches_only_its_blocks_of_a_host_destination(gpu, dev):
    w, h, count, block, shard = 40, 20, 3, 256, 1
    mine = (np.arange(w * h) // block) % count == shard
    assert mine.sum() == block and not mine[0] and not mine[-1]  # one whole block in the middle of four
    whole, _ = dev.run_raytracer(w, h, SPP, seed=3)
    fb = np.full(w * h * 3, 0x7FC00A5A, dtype=np.uint32).view(np.float32).reshape(h, w, 3)  # a NaN with a payload
    dev.run_raytracer(w, h, SPP, seed=3, shard_index=shard, shard_count=count, shard_block=block, out=fb)
    bits = fb.view(np.uint32).reshape(-1, 3)
    assert (bits[~mine] == 0x7FC00A5A).all()
    assert np.array_equal(bits[mine], whole.view(np.uint32).reshape(-1, 3)[mine])  # (device RNG: a pixel's samples do not depend on the sharding)
    whole8, _ = dev.run_raytracer_rgb8(w, h, SPP, seed=3)
    img = np.full((h, w, 3), 0xA5, dtype=np.uint8)
    dev.run_raytracer_rgb8(w, h, SPP, seed=3, shard_index=shard, shard_count=count, shard_block=block, out=img)
    assert (img.reshape(-1, 3)[~mine] == 0xA5).all() and np.array_equal(img.reshape(-1, 3)[mine], whole8.reshape(-1, 3)[mine])
