#!/usr/bin/env python3
"""Converged reference images for the denoiser's quality measurement (tests/test_denoise_quality.py, tools/denoise_quality.py): the CPU
oracle's 2048-SPP render of room_textured and room_manylights at 64 x 48 (device-RNG mode, seed 1001: not the seed of the 8-SPP images that are
measured against them). Written under tests/golden/denoise/ as float32 .npy (36 KB each). Only data is stored.
    python tests/golden/make_denoise_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import importlib  # noqa: E402

import oracle  # noqa: E402
from conftest import golden_scene_specs, make_scene  # noqa: E402

rt = importlib.import_module("raytracing-course-hw-public_amd")
OUT = os.path.join(HERE, "denoise")
W, H, SPP, SEED = 64, 48, 2048, 1001

if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    for name in ("room_textured", "room_manylights"):
        orc = oracle.OracleScene(make_scene(rt.scenegen, golden_scene_specs()[name]))
        fb, _ = orc.run_raytracer(W, H, SPP, seed=SEED, threads=min(16, os.cpu_count() or 1))
        np.save(os.path.join(OUT, f"ref_{name}_{W}x{H}x{SPP}.npy"), fb.astype(np.float32))
        print(name, fb.shape, float(fb.mean()))
        orc.close()
