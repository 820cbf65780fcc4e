#!/usr/bin/env python3
"""Stored answers of the UNMODIFIED reference for the "live" tests of tests/test_oracle_golden.py (container only, needs oracle/_ref).

Those tests used to run the reference binaries on the spot and skip where oracle/_ref is absent. Their answers are stored here, so they
run everywhere and re-run the reference live (checking these files) where it exists:
  * live/room900_40x56x3.ppm       the reference binary on room_scene(900, seed=777, ...) at 40x56, 3 SPP
  * live/room30000_96x64x2.ppm     the reference binary on room_scene(30000, seed=4711, ...) at 96x64, 2 SPP (a BVH ~20 levels deep)
  * live/bvh_room100k.sha256       sha256 of the reference BVH dump (ref_probe "bvh": scene tree, then light tree; per tree the uint32 words
                                   node count, object count, root, nodes (10 words each), object order) of room_scene(100000, seed=99, ...):
                                   the dump itself is 2.4 MB
  * live/lights2000_48x40x2.ppm    the reference binary on tests/deep_walks.py's volume_lights_scene(**BIG_LIGHTS): 2000 emissive triangles
                                   all through the room, a light tree of 2555 pieces (the other stored answers stop at 40 lights)
  * live/lights2000_lightpdf.npy   ref_probe "lightpdf" (bvh_mix_dist::pdf) on light_query_rays(scene, 2000, seed=77) of that scene: 2000 float32
  * live/needles20000_48x40x2.ppm  the reference binary on needle_soup_scene(emissive=True, **NEEDLES): 20 000 emissive needles, light queries
                                   with up to 14 subtrees pending
Scene parameters are the tests'. Only data is stored. Run:  python tests/golden/make_live_golden.py
"""
import hashlib
import importlib
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import oracle  # noqa: E402

import deep_walks  # noqa: E402

rt = importlib.import_module("raytracing-course-hw-public_amd")
sg = rt.scenegen
LIVE = os.path.join(HERE, "live")

RENDERS = {
    "room900_40x56x3.ppm": (dict(n_random=900, seed=777, n_lights=5, n_materials=7, tex_size=8, n_tex_sets=3, alpha_fraction=0.3, smooth_normals=True), 40, 56, 3),
    "room30000_96x64x2.ppm": (dict(n_random=30000, seed=4711, n_lights=6, n_materials=12, tex_size=16, n_tex_sets=4, alpha_fraction=0.1, offset=0.4), 96, 64, 2),
}
DEEP_RENDERS = {  # name -> (scene, width, height, samples)
    "lights2000_48x40x2.ppm": (lambda: deep_walks.volume_lights_scene(sg, **deep_walks.BIG_LIGHTS), 48, 40, 2),
    "needles20000_48x40x2.ppm": (lambda: deep_walks.needle_soup_scene(sg, emissive=True, **deep_walks.NEEDLES), 48, 40, 2),
}
LIGHTPDF = ("lights2000_lightpdf.npy", lambda: deep_walks.volume_lights_scene(sg, **deep_walks.BIG_LIGHTS), 2000, 77)  # name, scene, rays, ray seed
BVH_SCENE = dict(n_random=100000, seed=99, n_lights=20, n_materials=4, tex_size=0, offset=0.05)

if __name__ == "__main__":
    assert oracle.have_reference_build(), "build oracle/_ref first (make -C oracle)"
    os.makedirs(LIVE, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        for name, (spec, w, h, spp) in RENDERS.items():
            path = sg.write_gltf(sg.room_scene(**spec), os.path.join(td, "s.gltf"))
            oracle.run_reference(path, w, h, spp, os.path.join(td, "ref.ppm"))
            shutil.copyfile(os.path.join(td, "ref.ppm"), os.path.join(LIVE, name))
            print(name)
        for name, (make, w, h, spp) in DEEP_RENDERS.items():
            path = sg.write_gltf(make(), os.path.join(td, "d.gltf"))
            oracle.run_reference(path, w, h, spp, os.path.join(td, "ref.ppm"))
            shutil.copyfile(os.path.join(td, "ref.ppm"), os.path.join(LIVE, name))
            print(name)
        name, make, n_rays, ray_seed = LIGHTPDF
        sc = make()
        path = sg.write_gltf(sc, os.path.join(td, "lp.gltf"))
        deep_walks.light_query_rays(sc, n_rays, ray_seed).astype("<f4").tofile(os.path.join(td, "rays.bin"))
        oracle.ref_probe("lightpdf", path, 48, 40, os.path.join(td, "rays.bin"), os.path.join(td, "lp.bin"))
        np.save(os.path.join(LIVE, name), np.fromfile(os.path.join(td, "lp.bin"), dtype="<f4"))
        print(name)
        path = sg.write_gltf(sg.room_scene(**BVH_SCENE), os.path.join(td, "big.gltf"))
        oracle.ref_probe("bvh", path, 64, 48, os.path.join(td, "bvh.bin"))
        words = np.fromfile(os.path.join(td, "bvh.bin"), dtype=np.uint32)
        with open(os.path.join(LIVE, "bvh_room100k.sha256"), "w") as f:
            f.write(hashlib.sha256(words.tobytes()).hexdigest() + "\n")
        print("bvh_room100k.sha256", words.size, "words")
