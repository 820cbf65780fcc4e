"""Device memory over the life of one scene: the owners that the update leak tests (test_gpu_update_geometry.py) do not reach. Environments
are set, replaced and dropped, feature accumulators come and go with their denoiser workspace, rt_render_rays grows its ray buffer: free
device memory must stay where it was, and the scene must render what it rendered before any of it."""
import numpy as np
import pytest

from conftest import random_rays

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 64, 48, 1, 42
ENV_W, ENV_H = 256, 128
ROUNDS = 16
# The rule of test_updates_leak_no_device_memory: less than one environment texel buffer (16 B per texel, 512 KiB), where a leak of it per
# round would be 13 of them (6.5 MiB) between round 3 and round 16. The runtime hands device memory out in 2 MiB pieces, though: the commit
# BEFORE the device-memory owner types (rt_dev_mem.h) measured +2097152 bytes with this very test (an environment is live after round 3 and
# none is after round 16), so the bound is twice that measurement (profiles/dev_mem_bench.txt has both commits' figures). It is still
# below the 13 leaked buffers.
ENV_TEXELS_BYTES = ENV_W * ENV_H * 16
BOUND = 2 * 2097152
assert ENV_TEXELS_BYTES < BOUND < 13 * ENV_TEXELS_BYTES


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_environments_accumulators_and_ray_calls_leak_no_device_memory(gpu, scenes):
    import torch

    sc = scenes["room_manylights"]
    rng = np.random.default_rng(5)
    envs = [rng.uniform(0.0, 2.0, size=(ENV_H, ENV_W, 3)).astype(np.float32) for _ in range(2)]
    rays = random_rays(sc, 64, seed=9)
    dev = gpu.DeviceScene(sc)
    try:
        fb0 = dev.run_raytracer(W, H, SPP, seed=SEED)[0]
        free3 = None
        for i in range(ROUNDS):
            dev.set_environment(envs[i % 2], importance=(i % 2 == 0))
            acc = dev.accumulator(W, H, seed=SEED, features=True)
            try:
                acc.render(SPP)
                assert np.isfinite(acc.denoise()).all()
            finally:
                acc.close()
            out, _ = dev.render_rays(rays, seed=SEED)
            assert np.isfinite(out).all()
            if i % 4 == 3:
                dev.set_environment(None)
            if i == 2:
                free3 = torch.cuda.mem_get_info(0)[0]
        free16 = torch.cuda.mem_get_info(0)[0]
        print(f"free after round 3: {free3}, after round {ROUNDS}: {free16}, difference {free16 - free3}, one environment texel buffer: {ENV_TEXELS_BYTES}, bound: {BOUND}")
        assert abs(free16 - free3) < BOUND
        # round 16 dropped the environment: the scene is the one that rendered fb0
        assert np.array_equal(bits(dev.run_raytracer(W, H, SPP, seed=SEED)[0]), bits(fb0))
    finally:
        dev.close()
