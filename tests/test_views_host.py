"""CPU tests of the multi-view surface: the rt_view layout and rt_loaded_cameras (every camera of a file, as the loader computes the one
it keeps). The renders themselves are in test_gpu_views.py."""
import ctypes
import os
import subprocess

import numpy as np

from multiview import camera_words, desc_camera_words, three_camera_gltf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE000 = os.path.join(ROOT, "tests", "golden", "txt", "scene-000.txt")


def test_view_layout_matches_the_c_header(rt, tmp_path):
    abi = __import__("importlib").import_module("raytracing-course-hw-public_amd._ctypes_abi")
    src = tmp_path / "view.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\n'
                   'int main(){printf("%zu %zu %zu %zu\\n",sizeof(rt_view),offsetof(rt_view,camera),offsetof(rt_view,reserved),offsetof(rt_view,seed));return 0;}\n')
    exe = tmp_path / "view"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(abi.RtView), abi.RtView.camera.offset, abi.RtView.reserved.offset, abi.RtView.seed.offset]
    assert got[0] == 64 and got[3] == 56


def test_gltf_cameras_in_visit_order(rt, sg, tmp_path):
    path, variants = three_camera_gltf(sg, tmp_path)
    aspect = 64 / 48
    ls = rt.parse_gltf_scene(path, aspect)
    cams = ls.cameras()
    assert len(cams) == 3
    # the last camera is the one the reference keeps: the scene's camera, bit for bit
    assert np.array_equal(camera_words(cams[-1]), desc_camera_words(ls.desc))
    # camera i is what the loader makes of a file that holds camera node i alone (same transforms, other camera nodes removed)
    for i, vp in enumerate(variants):
        one = rt.parse_gltf_scene(vp, aspect)
        assert len(one.cameras()) == 1
        assert np.array_equal(camera_words(cams[i]), desc_camera_words(one.desc)), i
    # they differ: own position (parent transform), own fov (aspectRatio 1.5 vs the load's aspect), own yaw
    words = [camera_words(c) for c in cams]
    assert not np.array_equal(words[0], words[1]) and not np.array_equal(words[1], words[2]) and not np.array_equal(words[0], words[2])
    yfov, ar = np.float32(0.7), np.float32(1.5)
    assert cams[1].fov_x == float(np.float32(np.arctan(np.tan(yfov / np.float32(2)) * ar) * np.float32(2)))
    assert not np.allclose(cams[1].position, cams[0].position)


def test_gltf_cameras_count_query(rt, sg, tmp_path):
    path, _ = three_camera_gltf(sg, tmp_path)
    ls = rt.parse_gltf_scene(path, 1.0)
    n = ctypes.c_uint32(0)
    assert rt.lib().rt_loaded_cameras(ls._h, None, 0, ctypes.byref(n)) == 0 and n.value == 3
    one = (rt._ctypes_abi.RtCamera * 1)()
    assert rt.lib().rt_loaded_cameras(ls._h, one, 1, ctypes.byref(n)) == 0 and n.value == 3  # cap 1: the first camera only
    assert np.array_equal(camera_words(rt._camera_from_c(one[0])), camera_words(ls.cameras()[0]))
    assert rt.lib().rt_loaded_cameras(ls._h, None, 1, ctypes.byref(n)) != 0  # a capacity without a buffer


def test_scene_txt_has_one_camera(rt):
    ls = rt.parse_scene_txt(SCENE000)
    cams = ls.cameras()
    assert len(cams) == 1
    assert np.array_equal(camera_words(cams[0]), desc_camera_words(ls.desc))
