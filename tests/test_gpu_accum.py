"""GPU tests of the sample accumulators (include/rt_abi.h rt_accum_*): progressive and adaptive rendering. The contract is exact: after any
sequence of accumulator calls, pixel p of the resolved image is, bit for bit, pixel p of rt_render with samples = n_p (same scene, flags,
camera and seed), in the parity and production traversals, whatever max_paths, sort and packet mode, and however the samples were split."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_replay as ar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48
INVALID_ARG, UNSUPPORTED = 1, 8  # RT_ERR_*


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _window_max(err):
    """max of err over the 3x3 window around every pixel, clipped at the border; NaN counts as +inf (not converged)."""
    e = np.where(np.isnan(err), np.float32(np.inf), err)
    p = np.pad(e, 1, constant_values=-np.inf)
    h, w = e.shape
    return np.max(np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]), axis=0)


def _threshold_for(dev, mn, seed, frac=0.5, **kw):
    """A threshold at which about `frac` of the pixels have a clean window after min_samples: the count map comes out non-uniform."""
    probe = dev.accumulator(W, H, seed=seed)
    probe.render_adaptive(1e30, min_samples=mn, max_samples=mn, step=1, **kw)
    err = probe.read()["error"]
    probe.close()
    return float(np.float32(np.quantile(_window_max(err), frac)))


def _assert_exact_per_level(dev, img, n, seed, **kw):
    """Every pixel equals rt_render(samples = n_p) at that pixel; each distinct level is rendered once."""
    for lvl in np.unique(n):
        ref, _ = dev.run_raytracer(W, H, int(lvl), seed=seed, **kw)
        m = n == lvl
        assert np.array_equal(_bits(img[m]), _bits(ref[m])), int(lvl)


def _assert_error_matches_state(r):
    """err as the header defines it, recomputed from the read-back S, E and n: bit for bit the host model's binary32 err (adaptive_replay.err,
    the header's operations in its order, correctly rounded / and sqrt), and consistent with the formula in float64."""
    n = r["samples"]
    ok = n >= 2
    h = ((n + 1) // 2).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        I = r["sum"] / n.astype(np.float32)[..., None]
        A = r["even_sum"] / h[..., None]
        e64 = np.abs(I.astype(np.float64) - A.astype(np.float64)).sum(-1) / (1e-4 + np.sqrt(I.astype(np.float64).sum(-1)))
    err = r["error"].astype(np.float64)
    assert np.all(np.isinf(err[~ok]))
    fin = ok & np.isfinite(e64)
    assert np.allclose(err[fin], e64[fin], rtol=1e-5, atol=0.0)
    assert np.array_equal(np.isfinite(err[ok]), np.isfinite(e64[ok]))
    ar.assert_floats_equal(r["error"], ar.err(r["sum"], r["even_sum"], n), "err")


@pytest.mark.parametrize("mode", ["parity", "global_best", "wide"])
def test_progressive_equals_single_render(gpu, oracle, scenes, mode):
    sc = scenes["room_textured"]
    dev = gpu.DeviceScene(sc, **({"device_bvh": True, "wide": True} if mode == "wide" else {}))
    gb = mode != "parity"
    acc = dev.accumulator(W, H, seed=5)
    added = [acc.render(k, global_best=gb)["samples"] for k in (3, 5, 8)]
    assert added == [3 * W * H, 5 * W * H, 8 * W * H]
    img = acc.image()
    ref, _ = dev.run_raytracer(W, H, 16, seed=5, global_best=gb)
    assert np.array_equal(_bits(img), _bits(ref))
    if mode == "parity":
        ofb, _ = oracle.OracleScene(sc).run_raytracer(W, H, 16, rng_mode=gpu.RT_RNG_DEVICE, seed=5)
        assert np.array_equal(_bits(img), _bits(ofb))
    ref8, _ = dev.run_raytracer_rgb8(W, H, 16, seed=5, global_best=gb)
    assert np.array_equal(acc.image(rgb8=True), ref8)
    r = acc.read()
    assert np.all(r["samples"] == 16)
    dev.close()
    assert acc._h is None  # closed with its scene


def test_fresh_accumulator_resolves_to_zero(gpu, scenes):
    dev = gpu.DeviceScene(scenes["boxes"])
    acc = dev.accumulator(W, H)
    assert not np.any(acc.image()) and not np.any(acc.read()["samples"])
    assert np.all(np.isinf(acc.read()["error"]))
    dev.close()


def test_other_camera_and_seed_match_render_views(gpu, sg, scenes):
    sc = scenes["room_manylights"]
    cam = sg.look_camera(sc.camera.position, yaw_deg=25.0, yfov=0.7, aspect=W / H)
    dev = gpu.DeviceScene(sc)
    acc = dev.accumulator(W, H, camera=cam, seed=2024)
    acc.render(2)
    acc.render(4)
    ref, _ = dev.run_raytracer_views(W, H, 6, [cam], [2024])
    assert np.array_equal(_bits(acc.image()), _bits(ref[0]))
    own, _ = dev.run_raytracer(W, H, 6, seed=2024)
    assert not np.array_equal(own, ref[0])
    dev.close()


def test_state_independent_of_scheduling(gpu, scenes):
    sc = scenes["room_manylights"]
    dev = gpu.DeviceScene(sc)
    thr = _threshold_for(dev, 4, 3)
    variants = [
        dict(),
        dict(max_paths=1024, sort_mode=gpu.RT_SORT_OFF, packet_mode=gpu.RT_PACKET_OFF),
        dict(max_paths=1024, sort_mode=gpu.RT_SORT_OCTANT_CELL_CONE, packet_mode=gpu.RT_PACKET_ON),
        dict(sort_mode=gpu.RT_SORT_OCTANT_CELL_CONE, packet_mode=gpu.RT_PACKET_OFF),
    ]
    states, passes = [], []
    for tuning in variants:
        acc = dev.accumulator(W, H, seed=3)
        p0 = acc.render(3, **tuning)["passes"]
        p1 = acc.render_adaptive(thr, min_samples=4, max_samples=20, step=4, **tuning)["passes"]
        states.append(acc.read())
        passes.append(p0 + p1)
        acc.close()
    assert passes[1] > passes[0]  # max_paths = 1024 cut the lists into many passes
    for s in states[1:]:
        for k in ("sum", "even_sum", "samples", "error"):
            assert np.array_equal(_bits(s[k]), _bits(states[0][k])), k
    dev.close()


def test_adaptive_is_exact_and_keeps_its_invariant(gpu, scenes):
    sc = scenes["room_manylights"]
    dev = gpu.DeviceScene(sc)
    mn, mx, step, seed = 4, 32, 4, 9
    thr = _threshold_for(dev, mn, seed)
    acc = dev.accumulator(W, H, seed=seed)
    st = acc.render_adaptive(thr, min_samples=mn, max_samples=mx, step=step)
    r = acc.read()
    n = r["samples"]
    assert set(np.unique(n).tolist()) <= set(range(mn, mx + 1, step)) | {mx}
    assert mn < n.mean() < mx, n.mean()
    assert st["rounds"] >= 2 and st["samples"] == int(n.sum())
    _assert_exact_per_level(dev, acc.image(), n, seed)
    # after return: every pixel is at the cap or its whole window has converged, on the error that was read back
    assert np.all((n >= mx) | (_window_max(r["error"]) <= np.float32(thr)))
    _assert_error_matches_state(r)
    dev.close()


def test_edge_thresholds(gpu, scenes):
    sc = scenes["room_plain"]
    dev = gpu.DeviceScene(sc)
    mn, mx, seed = 4, 12, 1
    acc = dev.accumulator(W, H, seed=seed)
    acc.render_adaptive(0.0, min_samples=mn, max_samples=mx, step=4)
    r = acc.read()
    img = acc.image()
    # threshold 0: only a window whose every pixel has err exactly 0 (all samples equal) may stop below the cap
    below = r["samples"] < mx
    assert np.all(_window_max(r["error"])[below] == 0.0)
    if not below.any():
        ref, _ = dev.run_raytracer(W, H, mx, seed=seed)
        assert np.array_equal(_bits(img), _bits(ref))
    else:
        _assert_exact_per_level(dev, img, r["samples"], seed)
    acc.close()
    acc = dev.accumulator(W, H, seed=seed)
    st = acc.render_adaptive(3.0e38, min_samples=mn, max_samples=mx, step=4)
    assert st["rounds"] == 1 and np.all(acc.read()["samples"] == mn)
    ref, _ = dev.run_raytracer(W, H, mn, seed=seed)
    assert np.array_equal(_bits(acc.image()), _bits(ref))
    dev.close()


def test_round0_with_unequal_counts(gpu, scenes):
    sc = scenes["room_manylights"]
    dev = gpu.DeviceScene(sc, device_bvh=True, wide=True)
    seed = 4
    thr = _threshold_for(dev, 4, seed, global_best=True)
    acc = dev.accumulator(W, H, seed=seed)
    acc.render_adaptive(thr, min_samples=4, max_samples=16, step=4, global_best=True)
    n1 = acc.read()["samples"]
    assert (n1 == 4).any() and (n1 == 8).any()  # the second call's round 0 adds 8 to some pixels and 4 to others
    acc.render_adaptive(thr, min_samples=12, max_samples=16, step=4, global_best=True)
    r = acc.read()
    n2 = r["samples"]
    assert np.all(n2 >= 12) and np.all(n2 >= n1)
    _assert_exact_per_level(dev, acc.image(), n2, seed, global_best=True)
    assert np.all((n2 >= 16) | (_window_max(r["error"]) <= np.float32(thr)))
    dev.close()


def test_interleaved_render_leaves_the_accumulator_alone(gpu, scenes):
    sc = scenes["room_textured"]
    dev = gpu.DeviceScene(sc)
    acc = dev.accumulator(W, H, seed=21)
    acc.render(4)
    before = acc.read()
    # another size, seed and pass plan on the same scene: the workspace is resized and reused under the accumulator
    dev.run_raytracer(96, 80, 8, seed=77)
    dev.run_raytracer(W, H, 2, seed=5, max_paths=1024)
    after = acc.read()
    for k in before:
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k
    acc.render(4)
    ref, _ = dev.run_raytracer(W, H, 8, seed=21)
    assert np.array_equal(_bits(acc.image()), _bits(ref))
    dev.close()


def test_refusals(gpu, scenes):
    sc = scenes["boxes"]
    dev = gpu.DeviceScene(sc)
    acc = dev.accumulator(W, H)
    lib, abi = gpu.lib(), gpu._ctypes_abi

    def params(**kw):
        p = abi.RtParams(W, H, 4, abi.RT_RNG_DEVICE, 0, 0, 1, 0, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def render(p):
        return lib.rt_accum_render(acc._h, C.byref(p), None)

    def adaptive(p=None, **kw):
        ad = abi.RtAdaptive(0.1, 4, 16, 4)
        for k, v in kw.items():
            if k == "reserved2":
                ad.reserved[2] = v
            else:
                setattr(ad, k, v)
        return lib.rt_accum_render_adaptive(acc._h, C.byref(p or params()), C.byref(ad), None, None)

    assert render(params(rng_mode=abi.RT_RNG_REFERENCE)) == UNSUPPORTED
    assert render(params(flags=abi.RT_FLAG_MEGAKERNEL)) == UNSUPPORTED
    assert adaptive(params(rng_mode=abi.RT_RNG_REFERENCE)) == UNSUPPORTED
    assert render(params(width=W + 1)) == INVALID_ARG
    assert render(params(height=H - 1)) == INVALID_ARG
    assert render(params(samples=0)) == INVALID_ARG
    assert render(params(shard_count=2)) == INVALID_ARG
    assert render(params(flags=abi.RT_FLAG_DEVICE_FB)) == INVALID_ARG
    assert adaptive(params(width=W + 1)) == INVALID_ARG
    assert adaptive(min_samples=1) == INVALID_ARG
    assert adaptive(min_samples=8, max_samples=4) == INVALID_ARG
    assert adaptive(min_samples=0, max_samples=8) == INVALID_ARG  # 0 means 16
    assert adaptive(threshold=float("nan")) == INVALID_ARG
    assert adaptive(threshold=-1.0) == INVALID_ARG
    assert adaptive(threshold=float("inf")) == INVALID_ARG
    assert adaptive(reserved2=1) == INVALID_ARG
    assert lib.rt_accum_render_adaptive(acc._h, C.byref(params()), None, None, None) == INVALID_ARG
    assert lib.rt_accum_resolve(acc._h, abi.RT_FLAG_COUNTERS, None) == INVALID_ARG
    assert not np.any(acc.read()["samples"])  # nothing was rendered by a refused call
    assert adaptive() == 0
    grp = gpu.DeviceScene(sc, device=[0, 0], build_flags=gpu.RT_BUILD_GROUP_COPY)
    with pytest.raises(gpu.RtError) as e:
        grp.accumulator(W, H)
    assert e.value.code == UNSUPPORTED
    grp.close()
    dev.close()


def test_cli_adaptive(gpu, sg, tmp_path):
    sc = sg.room_scene(200, seed=31, n_lights=3, n_materials=4, tex_size=8, n_tex_sets=1)
    path = sg.write_gltf(sc, str(tmp_path / "room.gltf"))
    run = os.path.join(ROOT, "run.sh")
    env = dict(os.environ, RT_SEED="9", RT_DEVICE="0")
    plain, adapt = tmp_path / "plain.ppm", tmp_path / "adaptive.ppm"
    subprocess.check_call([run, path, str(W), str(H), "8", str(plain)], env=env)
    subprocess.check_call([run, path, str(W), str(H), "8", str(adapt)], env=dict(env, RT_ADAPTIVE="0"))
    assert adapt.read_bytes() == plain.read_bytes()
    # a real adaptive run: the count map, the verbose line, and every pixel the rgb8 render of its own count
    out, spp_map = tmp_path / "a24.ppm", tmp_path / "spp.pgm"
    res = subprocess.run([run, path, str(W), str(H), "24", str(out)], env=dict(env, RT_ADAPTIVE="0.05", RT_ADAPTIVE_MIN="4", RT_ADAPTIVE_STEP="4",
                                                                       RT_SPP_MAP=str(spp_map), RT_VERBOSE="1"), capture_output=True, text=True, check=True)
    assert "rounds=" in res.stderr and "mean_spp=" in res.stderr
    raw = spp_map.read_bytes()
    header = b"P5\n%d %d\n65535\n" % (W, H)
    assert raw.startswith(header)
    n = np.frombuffer(raw[len(header):], dtype=">u2").reshape(H, W)
    assert n.min() >= 4 and n.max() <= 24
    img = np.frombuffer(out.read_bytes()[-W * H * 3:], dtype=np.uint8).reshape(H, W, 3)
    ls = gpu.load_scene(path, W / H)
    dev = gpu.DeviceScene(ls)
    for lvl in np.unique(n):
        ref, _ = dev.run_raytracer_rgb8(W, H, int(lvl), seed=9)
        m = n == lvl
        assert np.array_equal(img[m], ref[m]), int(lvl)
    dev.close()
