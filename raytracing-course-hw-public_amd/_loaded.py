"""Scene files through the C++ host loaders (include/rt_host.h): glTF and scene-txt -> LoadedScene."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._ctypes_abi import RtCamera, RtSceneDesc, desc_to_arrays, fptr
from ._library import _check, lib
from ._sensors import _camera_from_c


class LoadedScene:
    """Result of parse_gltf_scene (scene.h:183) through the C++ host loader; owns the C-side arrays."""

    def __init__(self, handle: C.c_void_p):
        self._h = handle
        self.desc: RtSceneDesc = lib().rt_loaded_desc(handle).contents

    def arrays(self) -> dict:
        return desc_to_arrays(self.desc)

    def info(self) -> dict:
        """DIMENSIONS / SAMPLES of a scene-txt file (0 for glTF) and the number of ignored NEW_LIGHT blocks."""
        w, h, s, l = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().rt_loaded_info(self._h, C.byref(w), C.byref(h), C.byref(s), C.byref(l)))
        return {"width": w.value, "height": h.value, "samples": s.value, "ignored_lights": l.value}

    def cameras(self) -> list:
        """Every camera of the file as scenegen.Camera (rt_loaded_cameras): glTF camera nodes in the loader's visit order (the last is
        the scene's camera, the one the reference keeps), or the one camera of a scene-txt file."""
        n = C.c_uint32()
        _check(lib().rt_loaded_cameras(self._h, None, 0, C.byref(n)))
        arr = (RtCamera * max(1, n.value))()
        _check(lib().rt_loaded_cameras(self._h, arr, n.value, C.byref(n)))
        return [_camera_from_c(arr[i]) for i in range(n.value)]

    def set_env_map(self, image_path: str, intensity: float = 1.0) -> None:
        """main.cpp:28-31 under USE_ENV_MAP: scene.bg = Texture::load_img(image_path), bg_color = intensity (rt_loaded_set_env_map)."""
        _check(lib().rt_loaded_set_env_map(self._h, os.fsencode(image_path), C.c_float(intensity)))

    def disable_textures(self) -> None:
        """USE_TEXTURES = false (config.h:31-32): every texture lookup returns the texture's first texel (rt_loaded_disable_textures)."""
        _check(lib().rt_loaded_disable_textures(self._h))

    LIGHT_TRIANGLE_RELATIVE_POS = ((10.0, 0.0, -0.1), (0.0, 10.0, -0.1), (0.0, -10.0, -0.1))  # config.h:43-47

    def add_light_triangle(self, rel=LIGHT_TRIANGLE_RELATIVE_POS, intensity: float = 10.0) -> None:
        """scene.h:479-498 under ADD_LIGHT_TRIANGLE: an emissive triangle in the camera's frame (rt_loaded_add_light_triangle)."""
        r = np.ascontiguousarray(rel, dtype=np.float32).reshape(9)
        _check(lib().rt_loaded_add_light_triangle(self._h, fptr(r), C.c_float(intensity)))

    def close(self) -> None:
        if self._h:
            lib().rt_loaded_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _load(call) -> LoadedScene:
    h = C.c_void_p()
    _check(call(C.byref(h)))
    return LoadedScene(h)


def parse_gltf_scene(path: str, aspect: float) -> LoadedScene:
    return _load(lambda h: lib().rt_gltf_load(os.fsencode(path), C.c_float(aspect), h))


def parse_scene_txt(path: str) -> LoadedScene:
    """The scene-txt front end (csrc/host/txt_loader.cpp): sample_data-style scene files -> triangles + analytic primitives."""
    return _load(lambda h: lib().rt_txt_load(os.fsencode(path), h))


def load_scene(path: str, aspect: float) -> LoadedScene:
    """What the CLI does: scene-txt for *.txt, glTF otherwise (rt_scene_load)."""
    return _load(lambda h: lib().rt_scene_load(os.fsencode(path), C.c_float(aspect), h))
