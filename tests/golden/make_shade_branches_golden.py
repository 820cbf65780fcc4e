#!/usr/bin/env python3
"""Stored renders of the UNMODIFIED reference on the scenes of tests/shade_branches.py (container only, needs oracle/_ref).

tests/test_shade_census.py and tests/test_gpu_shade_branches.py hold the HIP kernels to the oracle on those scenes; these files hold the
oracle to the reference there: shade_branches.reference_scenes() are written as glTF (scenegen.write_gltf), rendered by the reference binary
with its own RNG at 32x24, 4 SPP, and the PPMs are stored under tests/golden/shade_branches/. reference_scenes' docstring says what a glTF
file cannot carry. Only data is stored. Run:  python tests/golden/make_shade_branches_golden.py
"""
import importlib
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import oracle  # noqa: E402

import shade_branches  # noqa: E402

rt = importlib.import_module("raytracing-course-hw-public_amd")
OUT = os.path.join(HERE, "shade_branches")

if __name__ == "__main__":
    assert oracle.have_reference_build(), "build oracle/_ref first (make -C oracle)"
    os.makedirs(OUT, exist_ok=True)
    w, h, spp = shade_branches.REFERENCE_RENDER
    with tempfile.TemporaryDirectory() as td:
        for name, sc in shade_branches.reference_scenes(rt.scenegen, rt).items():
            path = rt.scenegen.write_gltf(sc, os.path.join(td, name + ".gltf"))
            oracle.run_reference(path, w, h, spp, os.path.join(td, "ref.ppm"))
            shutil.copyfile(os.path.join(td, "ref.ppm"), os.path.join(OUT, shade_branches.reference_ppm_name(name)))
            print(shade_branches.reference_ppm_name(name))
