"""MI355X-native render loop for firelion9/raytracing-course-hw-public — Python host binding.

The product is the C-ABI shared library `csrc/librt_amd.so` (include/rt_abi.h + include/rt_host.h): hand-written
HIP kernels for gfx950 behind the seam the reference enters at `run_raytracer(scene, image)`
(src/raytracer.h:629). This package is a thin ctypes mirror of that ABI for tests and bench.py; names follow
the reference (`run_raytracer`, `parse_gltf_scene`, `Image.write`).

This file only gathers the names. The declarations are in _ctypes_abi, loading the library in _library, cameras in _sensors, scene files
in _loaded, packed records and scene descriptors in _records, DeviceScene in _device_scene, Accumulator in _accumulator, the functions
that need no GPU in _host, and the marshalling rules they all share in _marshal.

There is NO CPU fallback: if the library is missing, or no GPU is present when a device entry point is called,
the call raises.
"""
from __future__ import annotations

import ctypes as C  # noqa: F401 (this and the next five: names the package has always had)
import dataclasses  # noqa: F401
import os  # noqa: F401
from typing import Optional, Tuple  # noqa: F401

import numpy as np  # noqa: F401

from . import _library
from . import rays  # noqa: F401
from . import scenegen  # noqa: F401
from ._ctypes_abi import *  # noqa: F401,F403 (every declaration of the ABI mirror is a name of the package)
from ._library import LIB_PATH, RtError, _HERE, _check, device_count, lib
from ._sensors import Sensor, _camera_from_c, make_sensors, make_views
from ._loaded import LoadedScene, load_scene, parse_gltf_scene, parse_scene_txt
from ._records import GEOMETRY_ARRAYS, _as_desc, geometry_arrays, pack_bake_points, pack_rays
from ._marshal import _apply_tuning
from ._accumulator import Accumulator
from ._device_scene import DeviceScene
from ._host import bvh_build_host, bvh_wide_build_host, compact_derive_host, bvh_wide_refit_host, film_table, image_decode, load_hdr, png_decode, tonemap, write_flo, write_ppm


def __getattr__(name):
    if name == "_lib":  # the loaded library is _library's state: not copied here, where it would go stale
        return _library._lib
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = [
    "DeviceScene",
    "LoadedScene",
    "RT_ALL_DEVICES",
    "RT_RNG_DEVICE",
    "RT_RNG_REFERENCE",
    "RtError",
    "device_count",
    "lib",
    "parse_gltf_scene",
    "parse_scene_txt",
    "load_scene",
    "make_views",
    "make_sensors",
    "Sensor",
    "RtSensor",
    "RT_LIGHT_GROUP_MAX",
    "RT_LIGHT_GROUP_NONE",
    "pack_rays",
    "rays",
    "RAY_DTYPE",
    "RtRay",
    "pack_bake_points",
    "BAKE_POINT_DTYPE",
    "RtBakePoint",
    "RtBake",
    "RT_BAKE_IRRADIANCE",
    "RT_BAKE_SH9",
    "load_hdr",
    "png_decode",
    "scenegen",
    "tonemap",
    "write_ppm",
]
