"""rt_accum_denoise against its host model (tests/denoise_replay.py), bit for bit: the model is fed with the accumulator's own read-back state,
so every difference is the filter's. Sizes that no tile divides and that clip every stride at the borders, 1 x 1 and 5 x 3 images, 1 to 5
iterations (LDS tiles at strides 1 and 2, gathers from 4 on), with and without demodulation, on an uneven count map and on a state where
every pixel holds one sample (filtered by geometry alone)."""
import os
import subprocess

import numpy as np
import pytest

import denoise_replay as dr
import feature_replay as fr

pytestmark = pytest.mark.gpu

SEED = 7


@pytest.fixture(scope="module")
def devs(gpu, scenes):
    d = {name: gpu.DeviceScene(scenes[name]) for name in ("room_textured", "open_nolight")}
    yield d
    for dev in d.values():
        dev.close()


def _uneven(acc):
    """n_p from 2 to 8: round 0 brings every pixel to 2, later rounds add one sample where the window has not converged."""
    acc.render(1)
    e = acc._scene.accumulator(acc.width, acc.height, seed=SEED)
    e.render(2)
    e.render_adaptive(0.0, min_samples=2, max_samples=2, step=1)
    err = e.read()["error"]
    e.close()
    pos = err[np.isfinite(err) & (err > 0)]  # an open scene is mostly background with err exactly 0: the threshold comes from the pixels that vary
    acc.render_adaptive(float(np.median(pos)) if len(pos) else 0.0, min_samples=2, max_samples=8, step=1)
    return acc.read()["samples"]


@pytest.mark.parametrize("shape", [(67, 45), (64, 48), (1, 1), (5, 3)])  # (width, height)
@pytest.mark.parametrize("scene", ["room_textured", "open_nolight"])
def test_denoise_is_the_model(devs, scene, shape):
    w, h = shape
    dev = devs[scene]
    for state in ("one_sample", "uneven"):
        acc = dev.accumulator(w, h, seed=SEED, features=True)
        if state == "one_sample":
            acc.render(1)
            assert np.all(acc.read()["samples"] == 1)
        else:
            n = _uneven(acc)
            levels = len(np.unique(n))
            print(f"{scene} {w}x{h}: count levels {np.unique(n).tolist()}")
            assert n.min() >= 2 and n.max() <= 8 and (w * h < 100 or levels >= (3 if scene == "room_textured" else 2))
        for K in (1, 3, 5):
            for demod in (True, False):
                got = acc.denoise(iterations=K, demodulate=demod)
                want = dr.of_accumulator(acc, iterations=K, demodulate=demod)
                fr.assert_bits(got, want, f"{scene} {w}x{h} {state} K={K} demodulate={demod}")
        acc.close()


def test_options_reach_the_kernels(devs):
    acc = devs["room_textured"].accumulator(67, 45, seed=SEED, features=True)
    _uneven(acc)
    base = acc.denoise()
    fr.assert_bits(base, dr.of_accumulator(acc), "defaults")
    assert np.abs(base - acc.image()).max() > 1e-3  # it filters
    for opts in (dict(sigma_color=0.5), dict(sigma_depth=0.05), dict(normal_sharpness=1), dict(iterations=8), dict(sigma_color=16.0, sigma_depth=2.0, normal_sharpness=6)):
        got = acc.denoise(**opts)
        fr.assert_bits(got, dr.of_accumulator(acc, **opts), str(opts))
        assert not fr.same_bits(got, base), opts
    acc.close()


def test_rgb8_twice_and_state_untouched(gpu, devs):
    import ctypes as C

    import torch

    acc = devs["open_nolight"].accumulator(67, 45, seed=SEED, features=True)
    _uneven(acc)
    before, fbefore = acc.read(), acc.read_features()
    a = acc.denoise()
    assert np.array_equal(acc.denoise(rgb8=True), gpu.tonemap(a))
    b = acc.denoise()
    assert fr.same_bits(a, b)
    after, fafter = acc.read(), acc.read_features()
    for k in before:
        assert fr.same_bits(before[k], after[k]), k
    for k in fbefore:
        assert fr.same_bits(fbefore[k], fafter[k]), k
    # device destinations
    lib, abi = gpu.lib(), gpu._ctypes_abi
    fb = torch.full((45 * 67 * 3,), -1.0, dtype=torch.float32, device="cuda")
    al = torch.full((45 * 67 * 3,), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert lib.rt_accum_denoise(acc._h, None, abi.RT_FLAG_DEVICE_FB, C.c_void_p(fb.data_ptr())) == 0
    assert lib.rt_accum_resolve_features(acc._h, abi.RT_FLAG_DEVICE_FB, C.c_void_p(al.data_ptr()), None, None) == 0
    assert fr.same_bits(fb.cpu().numpy().reshape(45, 67, 3), a)
    assert fr.same_bits(al.cpu().numpy().reshape(45, 67, 3), acc.features()["albedo"])
    # denoise, add samples, denoise again
    acc.render(2)
    fr.assert_bits(acc.denoise(), dr.of_accumulator(acc), "after more samples")
    acc.close()


def _read_pfm(path):
    with open(path, "rb") as f:
        data = f.read()
    kind, dims, scale, body = data.split(b"\n", 3)
    assert kind == b"Pf" and float(scale) < 0
    w, h = (int(x) for x in dims.split())
    return np.frombuffer(body, dtype="<f4").reshape(h, w)[::-1]  # rows bottom to top


def _quantise(x):
    return (np.clip(x.astype(np.float32), np.float32(0), np.float32(1)) * np.float32(255) + np.float32(0.5)).astype(np.uint8)


def test_cli_denoise_and_aov(gpu, oracle, tmp_path):
    from conftest import SCENE000

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    W, H, SPP = 64, 48, 4
    out, prefix = tmp_path / "dn.ppm", tmp_path / "aov"
    subprocess.check_call([os.path.join(root, "run.sh"), SCENE000, str(W), str(H), str(SPP), str(out)],
                          env=dict(os.environ, RT_DENOISE="1", RT_AOV=str(prefix), RT_SEED="17", RT_DEVICE="0"))
    ls = gpu.parse_scene_txt(SCENE000)
    dev = gpu.DeviceScene(ls)
    acc = dev.accumulator(W, H, seed=17, features=True)
    acc.render(SPP)
    assert np.array_equal(oracle.read_ppm(str(out)), acc.denoise(rgb8=True))
    f = acc.features()
    assert np.array_equal(oracle.read_ppm(f"{prefix}_albedo.ppm"), _quantise(f["albedo"]))
    assert np.array_equal(oracle.read_ppm(f"{prefix}_normal.ppm"), _quantise(np.float32(0.5) * f["normal"] + np.float32(0.5)))
    assert fr.same_bits(np.ascontiguousarray(_read_pfm(f"{prefix}_depth.pfm")), f["depth"])
    assert f["depth"].max() > 0 and len(np.unique(_quantise(f["albedo"]).reshape(-1, 3), axis=0)) >= 2
    # RT_AOV alone: the plain image of the same accumulator
    out2 = tmp_path / "plain.ppm"
    subprocess.check_call([os.path.join(root, "run.sh"), SCENE000, str(W), str(H), str(SPP), str(out2)],
                          env=dict(os.environ, RT_AOV=str(tmp_path / "aov2"), RT_SEED="17", RT_DEVICE="0"))
    assert np.array_equal(oracle.read_ppm(str(out2)), acc.image(rgb8=True))
    acc.close()
    dev.close()
