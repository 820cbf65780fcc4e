"""Shared scenes of the multi-view tests (test_views_host.py, test_gpu_views.py): a glTF file with three camera nodes, one of them under
a parent transform and one with its own aspectRatio, and variants of it that keep one camera node each."""
import copy
import json
import os

import numpy as np


def three_camera_gltf(sg, out_dir, name="views3"):
    """(path of the 3-camera file, [path of the variant holding only camera node i, for i in visit order])."""
    sc = sg.room_scene(200, seed=31, n_lights=3, n_materials=4, tex_size=8, n_tex_sets=1)
    sc.camera = sg.look_camera(sc.camera.position, yaw_deg=0.0, yfov=0.9)
    base = sg.write_gltf(sc, os.path.join(str(out_dir), name + ".gltf"))
    doc = json.load(open(base))
    pos = [float(x) for x in sc.camera.position]
    q = np.float32(np.sin(np.deg2rad(20.0) / 2)), np.float32(np.cos(np.deg2rad(20.0) / 2))
    doc["cameras"] = [
        {"type": "perspective", "perspective": {"yfov": 0.9, "znear": 0.01}},
        {"type": "perspective", "perspective": {"yfov": 0.7, "aspectRatio": 1.5, "znear": 0.01}},
        {"type": "perspective", "perspective": {"yfov": 1.1, "znear": 0.01}},
    ]
    doc["nodes"] = [
        doc["nodes"][0],  # the mesh
        {"camera": 0, "translation": pos, "rotation": [0.0, float(q[0]), 0.0, float(q[1])]},
        {"translation": [0.25, 0.1, -0.2], "rotation": [0.0, -float(q[0]), 0.0, float(q[1])], "scale": [1.0, 1.0, 1.0], "children": [3]},  # parent
        {"camera": 1, "translation": pos, "rotation": [0.0, 0.0, 0.0, 1.0]},
        {"camera": 2, "translation": [pos[0] - 0.3, pos[1], pos[2] + 0.2], "rotation": [0.0, -float(q[0]), 0.0, float(q[1])]},
    ]
    doc["scenes"] = [{"nodes": [0, 1, 2, 4]}]
    path = os.path.join(str(out_dir), name + "_all.gltf")
    json.dump(doc, open(path, "w"))
    variants = []
    for i, keep in enumerate((1, 3, 4)):  # the camera nodes in visit order
        d = copy.deepcopy(doc)
        for k, node in enumerate(d["nodes"]):
            if "camera" in node and k != keep:
                del node["camera"]
        vp = os.path.join(str(out_dir), f"{name}_only{i}.gltf")
        json.dump(d, open(vp, "w"))
        variants.append(vp)
    return path, variants


def camera_words(cam):
    """The camera's 13 floats as u32 words (bitwise comparison)."""
    f = np.concatenate([np.asarray(cam.position, np.float32), np.asarray(cam.right, np.float32), np.asarray(cam.up, np.float32),
                        np.asarray(cam.forward, np.float32), np.array([cam.fov_x], np.float32)])
    return f.view(np.uint32)


def desc_camera_words(desc):
    c = desc.camera
    f = np.array(list(c.position) + list(c.right) + list(c.up) + list(c.forward) + [c.fov_x], dtype=np.float32)
    return f.view(np.uint32)
