"""ctypes binding of the CPU oracle (oracle/liboracle.so, oracle/rt_oracle.cpp).

TEST INFRASTRUCTURE: imported only by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg.
The oracle consumes the same rt_scene_desc structs as the product ABI (include/rt_abi.h).
"""
from __future__ import annotations

import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
_abi = importlib.import_module("raytracing-course-hw-public_amd._ctypes_abi")

LIB_PATH = os.path.join(_HERE, "liboracle.so")
REF_DIR = os.path.join(_HERE, "_ref")
REF_BINARY = os.path.join(REF_DIR, "raytracer_ref")
REF_PROBE = os.path.join(REF_DIR, "ref_probe")
STDRAND_PROBE = os.path.join(REF_DIR, "stdrand_probe")

_lib = None

_PROTOS = {
    "rto_create": (C.c_int, [C.POINTER(_abi.RtSceneDesc), C.POINTER(C.c_void_p)]),
    "rto_destroy": (None, [C.c_void_p]),
    "rto_render": (C.c_int, [C.c_void_p, C.POINTER(_abi.RtParams), _abi.c_float_p, C.POINTER(_abi.RtStats), C.c_int]),
    "rto_cast_rays": (C.c_int, [C.c_void_p, _abi.c_float_p, C.c_uint32, _abi.c_u32_p, _abi.c_float_p]),
    "rto_intersect_objects": (C.c_int, [C.c_void_p, _abi.c_float_p, C.c_uint32, _abi.c_u32_p, _abi.c_u32_p, _abi.c_float_p]),
    "rto_cast_rays_brute": (C.c_int, [C.c_void_p, _abi.c_float_p, C.c_uint32, _abi.c_u32_p, _abi.c_float_p, C.c_int]),
    "rto_trace_pixel": (C.c_int, [C.c_void_p, C.POINTER(_abi.RtParams), C.c_uint32, C.c_uint32, _abi.c_float_p, _abi.c_u32_p, _abi.c_u32_p]),
    "rto_pixel_samples": (C.c_int, [C.c_void_p, C.POINTER(_abi.RtParams), _abi.c_u32_p, C.c_uint32, _abi.c_float_p, C.c_int]),
    "rto_trace_rays": (C.c_int, [C.c_void_p, C.POINTER(_abi.RtParams), C.c_void_p, C.c_uint32, _abi.c_float_p, C.POINTER(_abi.RtStats), C.c_int]),
    "rto_shade_census": (C.c_int, [C.c_void_p, C.POINTER(_abi.RtParams), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.c_int]),
    "rto_shade_slot_count": (C.c_uint32, []),
    "rto_shade_slot_name": (C.c_char_p, [C.c_uint32]),
    "rto_light_pdf": (C.c_int, [C.c_void_p, _abi.c_float_p, C.c_uint32, _abi.c_float_p]),
    "rto_walk_census": (C.c_int, [C.c_void_p, _abi.c_float_p, C.c_uint32, _abi.c_u32_p, _abi.c_u32_p]),
    "rto_dump_census": (C.c_int, [_abi.c_u32_p, C.c_uint32, _abi.c_u32_p, C.c_uint32, C.c_uint32, _abi.c_float_p, C.c_uint32, _abi.c_u32_p]),
    "rto_wide_census": (C.c_int, [_abi.c_u32_p, C.c_uint32, _abi.c_u32_p, C.c_uint32, _abi.c_float_p, C.c_uint32, _abi.c_float_p, C.c_uint32, _abi.c_u32_p]),
    "rto_bg_at": (C.c_int, [C.c_void_p, _abi.c_float_p, C.c_uint32, _abi.c_float_p]),
    "rto_bg_uv": (None, [_abi.c_float_p, C.c_uint32, C.c_int, _abi.c_float_p]),
    "rto_bvh_info": (C.c_int, [C.c_void_p, C.c_int, _abi.c_u32_p, _abi.c_u32_p, _abi.c_u32_p, _abi.c_u32_p, _abi.c_u32_p]),
    "rto_tonemap_rgb8": (None, [_abi.c_float_p, C.c_size_t, _abi.c_u8_p]),
    "rto_last_error": (C.c_char_p, []),
    "rto_minstd_sequence": (None, [C.c_uint32, C.c_uint32, _abi.c_float_p]),
    "rto_minstd_below_sequence": (None, [C.c_uint32, C.c_uint32, C.c_uint32, _abi.c_u32_p]),
    "rto_sincos": (None, [_abi.c_float_p, C.c_uint32, _abi.c_float_p, _abi.c_float_p]),
    "rto_libm_sincos": (None, [_abi.c_float_p, C.c_uint32, _abi.c_float_p, _abi.c_float_p]),
    "rto_xoshiro_sequence": (None, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _abi.c_float_p]),
    "rto_xoshiro_raw": (None, [_abi.c_u32_p, C.c_uint32, _abi.c_u32_p]),
    "rto_xoshiro_below_sequence": (None, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _abi.c_u32_p]),
}


# The shade census' slots, in the order of RTO_SHADE_SLOTS in rt_oracle.cpp (lib() checks that the two tables agree). tex_*: Texture::sample's
# footprint kinds, once for lookups with gamma and once without; surf_*: to_intersection_info; shade_* / light_*: shade; vndf_* / local_x_* /
# brdf_* / spec_*: vndf_sample, vndf_pdf and the BRDF; trace_*: trace_ray; sanitize_*: sanitize_nans.
_TEX_KINDS = ("tex_1x1", "tex_inside", "tex_x1_wraps", "tex_y1_wraps", "tex_u_up_inside", "tex_u_up_last_row", "tex_v_up", "tex_both_up", "tex_w1_x1_is_2")
SHADE_SLOTS = tuple(f"{k}_gamma" for k in _TEX_KINDS) + tuple(f"{k}_linear" for k in _TEX_KINDS) + (
    "surf_inside", "surf_outside", "surf_smooth_flipped", "surf_smooth_kept", "surf_shading_nan", "surf_shading_finite", "surf_analytic", "surf_triangle",
    "shade_alpha_pass", "shade_alpha_scatter", "shade_vndf", "shade_cosine_no_lights", "shade_mix_cosine", "shade_mix_light",
    "light_folded", "light_not_folded", "shade_nan_dir_exit", "shade_dir_finite", "shade_p_lt_eps_exit", "shade_p_ok", "shade_scl_zero_exit", "shade_push",
    "vndf_lensq_pos", "vndf_lensq_zero", "local_x_arm_x", "local_x_arm_y", "local_x_arm_z", "vndf_pdf_vdn_le_0", "vndf_pdf_vdn_pos",
    "brdf_metallic_0", "brdf_metallic_1", "brdf_metallic_between", "brdf_rough_clamped", "brdf_rough_kept",
    "spec_ndh_zero", "spec_ndh_one", "spec_hdo_zero", "spec_hdo_one", "spec_hdi_zero", "spec_hdi_one",
    "trace_miss_background", "trace_depth_exhausted", "sanitize_x", "sanitize_y", "sanitize_z")


def build() -> None:
    subprocess.check_call(["make", "-C", _HERE, "all"], stdout=subprocess.DEVNULL)


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        _lib = C.CDLL(LIB_PATH)
        _abi.bind(_lib, _PROTOS)
        names = tuple(_lib.rto_shade_slot_name(i).decode() for i in range(_lib.rto_shade_slot_count()))
        assert names == SHADE_SLOTS, "oracle.SHADE_SLOTS and RTO_SHADE_SLOTS (rt_oracle.cpp) differ"
    return _lib


def _check(code: int) -> None:
    if code != 0:
        raise RuntimeError(f"oracle error {code}: {lib().rto_last_error().decode()}")


def have_reference_build() -> bool:
    return os.path.exists(REF_BINARY) and os.path.exists(REF_PROBE)


def _pack_rays(rays, stream=None, first_sample=None):
    """RAY_DTYPE records: a packed array as it is, an (n, 6) float array with `stream` (default: the index) and `first_sample` (default 0)."""
    if isinstance(rays, np.ndarray) and rays.dtype == _abi.RAY_DTYPE:
        assert stream is None and first_sample is None, "packed rays carry their own stream / first_sample"
        return np.ascontiguousarray(rays).reshape(-1)
    od = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    out = np.zeros(od.shape[0], dtype=_abi.RAY_DTYPE)
    out["origin"], out["dir"] = od[:, :3], od[:, 3:]
    out["stream"] = np.arange(od.shape[0], dtype=np.uint32) if stream is None else np.asarray(stream, dtype=np.uint32).reshape(-1)
    out["first_sample"] = 0 if first_sample is None else np.asarray(first_sample, dtype=np.uint32).reshape(-1)
    return out


class OracleScene:
    def __init__(self, scene):
        if isinstance(scene, _abi.RtSceneDesc):
            desc, self._keep = scene, None
        elif hasattr(scene, "desc") and isinstance(scene.desc, _abi.RtSceneDesc):
            desc, self._keep = scene.desc, scene
        else:
            self._keep = _abi.DescHolder(scene)
            desc = self._keep.desc
        self._h = C.c_void_p()
        _check(lib().rto_create(C.byref(desc), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().rto_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run_raytracer(self, width, height, samples, rng_mode=_abi.RT_RNG_DEVICE, seed=0, shard_index=0, shard_count=1,
                      shard_block=0, threads=0, out=None):
        """CPU restatement of run_raytracer (raytracer.h:629): the reference's arithmetic (libm included) in both RNG modes; the
        modes differ in the random stream only."""
        p = _abi.RtParams(width, height, samples, rng_mode, seed, shard_index, shard_count, shard_block, 0)
        st = _abi.RtStats()
        fb = out if out is not None else np.zeros((height, width, 3), dtype=np.float32)
        _check(lib().rto_render(self._h, C.byref(p), _abi.fptr(fb), C.byref(st), int(threads)))
        return fb, st.as_dict()

    def cast_rays(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        prim = np.zeros(n, dtype=np.uint32)
        bct = np.zeros((n, 3), dtype=np.float32)
        _check(lib().rto_cast_rays(self._h, _abi.fptr(rays), n, _abi.u32ptr(prim), _abi.fptr(bct)))
        return prim, bct

    def intersect_objects(self, rays, objs):
        """Ray i against object objs[i] only (a triangle through the BVH walk's own test, an index >= n_triangles as an analytic primitive,
        reported (0, 0, t)): (hit flags (n,) bool, bct (n, 3) float32, zero where not hit)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        objs = np.ascontiguousarray(objs, dtype=np.uint32).reshape(-1)
        n = rays.shape[0]
        assert objs.shape[0] == n
        hit = np.zeros(n, dtype=np.uint32)
        bct = np.zeros((n, 3), dtype=np.float32)
        _check(lib().rto_intersect_objects(self._h, _abi.fptr(rays), n, _abi.u32ptr(objs), _abi.u32ptr(hit), _abi.fptr(bct)))
        return hit != 0, bct

    def cast_rays_brute(self, rays, threads=None):
        """The closest hit over ALL objects without a tree (update_intersection's rule: strictly smaller t wins, the first index on equal t;
        primitives as in cast_rays): (prim, bct) like cast_rays. `threads`: worker count, by default min(16, OMP_NUM_THREADS or 16)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        if threads is None:
            threads = min(16, int(os.environ.get("OMP_NUM_THREADS") or 16))
        prim = np.zeros(n, dtype=np.uint32)
        bct = np.zeros((n, 3), dtype=np.float32)
        _check(lib().rto_cast_rays_brute(self._h, _abi.fptr(rays), n, _abi.u32ptr(prim), _abi.fptr(bct), max(1, int(threads))))
        return prim, bct

    def trace_pixel(self, width, height, samples, pixel, seed=0):
        """The rays the samples of one pixel cast (device-RNG mode), in cast order: (rays (n, 6) float32, sample index per ray)."""
        p = _abi.RtParams(width, height, samples, _abi.RT_RNG_DEVICE, seed, 0, 1, 0, 0)
        n = C.c_uint32()
        cap = samples * 64
        rays = np.zeros((cap, 6), dtype=np.float32)
        smp = np.zeros(cap, dtype=np.uint32)
        _check(lib().rto_trace_pixel(self._h, C.byref(p), int(pixel), cap, _abi.fptr(rays), _abi.u32ptr(smp), C.byref(n)))
        assert n.value <= cap
        return rays[: n.value].copy(), smp[: n.value].copy()

    def pixel_samples(self, width, height, samples, pixels, seed=0, threads=None):
        """Every sample's radiance for the listed pixel indices (device-RNG mode, the scene's camera): (len(pixels), samples, 3) float32, the
        value render_pixel adds for sample s of each pixel (after sanitize_nans), seeded by (seed, pixel, s). `threads`: as cast_rays_brute."""
        pixels = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
        if threads is None:
            threads = min(16, int(os.environ.get("OMP_NUM_THREADS") or 16))
        p = _abi.RtParams(width, height, samples, _abi.RT_RNG_DEVICE, seed, 0, 1, 0, 0)
        out = np.zeros((len(pixels), samples, 3), dtype=np.float32)
        _check(lib().rto_pixel_samples(self._h, C.byref(p), _abi.u32ptr(pixels), len(pixels), _abi.fptr(out), max(1, int(threads))))
        return out

    def trace_rays(self, rays, samples, seed=0, threads=None, stream=None, first_sample=None):
        """rt_render_rays' values before the fold (include/rt_abi.h, "The rule, operation by operation"): for ray r and sample s < samples,
        sanitize_nans(trace_ray(r, ray_depth)) seeded from (seed, r.stream, r.first_sample + s) after two discarded draws. `rays`: RAY_DTYPE
        records, or an (n, 6) float array with `stream` / `first_sample` arrays (by default stream = index, first_sample = 0). Returns ((n, samples, 3) float32, the event counters as run_raytracer returns them). `threads`: as cast_rays_brute."""
        packed = _pack_rays(rays, stream, first_sample)
        if threads is None:
            threads = min(16, int(os.environ.get("OMP_NUM_THREADS") or 16))
        p = _abi.RtParams(0, 0, int(samples), _abi.RT_RNG_DEVICE, int(seed), 0, 1, 0, 0)
        st = _abi.RtStats()
        out = np.zeros((len(packed), int(samples), 3), dtype=np.float32)
        _check(lib().rto_trace_rays(self._h, C.byref(p), packed.ctypes.data_as(C.c_void_p), len(packed), _abi.fptr(out), C.byref(st), max(1, int(threads))))
        return out, st.as_dict()

    def _census(self, p, packed):
        counts = (C.c_uint64 * len(SHADE_SLOTS))()
        ptr, n = (packed.ctypes.data_as(C.c_void_p), len(packed)) if packed is not None else (None, 0)
        _check(lib().rto_shade_census(self._h, C.byref(p), ptr, n, counts, min(16, int(os.environ.get("OMP_NUM_THREADS") or 16))))
        return {name: int(counts[i]) for i, name in enumerate(SHADE_SLOTS)}

    def shade_census(self, rays, samples, seed=0, stream=None, first_sample=None):
        """{slot name: events} over the samples trace_rays(rays, samples, seed) traces: how often each side of each branch of the shading
        path (SHADE_SLOTS) is taken. A replay that changes and returns nothing else."""
        packed = _pack_rays(rays, stream, first_sample)
        return self._census(_abi.RtParams(0, 0, int(samples), _abi.RT_RNG_DEVICE, int(seed), 0, 1, 0, 0), packed)

    def shade_census_render(self, width, height, samples, seed=0, rng_mode=_abi.RT_RNG_DEVICE):
        """The same census over the samples of run_raytracer(width, height, samples, rng_mode, seed)."""
        return self._census(_abi.RtParams(width, height, samples, rng_mode, seed, 0, 1, 0, 0), None)

    def light_pdf(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        out = np.zeros(rays.shape[0], dtype=np.float32)
        _check(lib().rto_light_pdf(self._h, _abi.fptr(rays), rays.shape[0], _abi.fptr(out)))
        return out

    def walk_census(self, rays):
        """Per ray, the largest number of deferred far siblings pending at once: (closest (n,) uint32 for intersect_ray on the scene tree,
        light (n,) uint32 for foreach_intersection on the light tree with the ray as (x, d) of light_pdf). A traversal stack holds exactly
        these, so the counts say which tier of a two-tier stack a ray reaches."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        closest = np.zeros(n, dtype=np.uint32)
        light = np.zeros(n, dtype=np.uint32)
        _check(lib().rto_walk_census(self._h, _abi.fptr(rays), n, _abi.u32ptr(closest), _abi.u32ptr(light)))
        return closest, light

    def bg_at(self, dirs):
        """Scene::bg_at (scene.h:83-89) for explicit directions -> (n, 3) rgb."""
        dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((dirs.shape[0], 3), dtype=np.float32)
        _check(lib().rto_bg_at(self._h, _abi.fptr(dirs), dirs.shape[0], _abi.fptr(out)))
        return out

    def bvh_info(self, which):
        nn, no, root = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().rto_bvh_info(self._h, which, C.byref(nn), C.byref(no), C.byref(root), None, None))
        nodes = np.zeros((nn.value, 10), dtype=np.uint32)
        order = np.zeros(no.value, dtype=np.uint32)
        _check(lib().rto_bvh_info(self._h, which, C.byref(nn), C.byref(no), C.byref(root), _abi.u32ptr(nodes), _abi.u32ptr(order)))
        return {"root": root.value, "nodes": nodes, "order": order}


def dump_census(dump, rays):
    """walk_census's closest-hit count for a binary tree given as the records the device holds (DeviceScene.bvh_device_dump: {root, nodes
    (n, 16) uint32, tris (n, 12) uint32}): per ray, the largest number of deferred siblings pending at once when the reference's closest-hit
    recursion walks THAT tree (rto_dump_census). The way to a census of trees the reference builder does not build."""
    nodes = np.ascontiguousarray(dump["nodes"], dtype=np.uint32).reshape(-1, 16)
    tris = np.ascontiguousarray(dump["tris"], dtype=np.uint32).reshape(-1, 12)
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    out = np.zeros(rays.shape[0], dtype=np.uint32)
    _check(lib().rto_dump_census(_abi.u32ptr(nodes), nodes.shape[0], _abi.u32ptr(tris), tris.shape[0], int(dump["root"]), _abi.fptr(rays), rays.shape[0],
                                 _abi.u32ptr(out)))
    return out


def wide_census(nodes80, order, positions, rays):
    """The census of the 8-wide walk (rto_wide_census): per ray, the largest number of node groups pending at once when the rule of
    csrc/rt_wide.hip's wide_node_step walks 80-byte WideNode records, `nodes80` (n, 20) uint32 of bvh_wide_build_host or
    DeviceScene.bvh_wide_dump. order[k]: the triangle of triangle record k; positions: the scene's (n_triangles, 9) float32. Boxes are tested in
    float64 on the de-quantised planes, triangles by the oracle's own test; tests/deep_walks.py wide_census states the rule in full."""
    nodes = np.ascontiguousarray(nodes80, dtype=np.uint32).reshape(-1, 20)
    order = np.ascontiguousarray(order, dtype=np.uint32).reshape(-1)
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 9)
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    out = np.zeros(rays.shape[0], dtype=np.uint32)
    _check(lib().rto_wide_census(_abi.u32ptr(nodes), nodes.shape[0], _abi.u32ptr(order), order.shape[0], _abi.fptr(pos), pos.shape[0], _abi.fptr(rays),
                                 rays.shape[0], _abi.u32ptr(out)))
    return out


def fold_outputs(per_sample, rays_per_output=1):
    """rt_render_rays' output rule in float32 (render_pixel's loop, raytracer.h:618-627): `per_sample` is (n_rays, K, 3), or a sequence of
    equal-shaped arrays to be added in that order; output j starts from +0.0, adds the values of rays j*G .. j*G + G - 1 in that order, each
    ray's K samples in sample order, and is divided by (float)(G * K). Returns (n_rays / G, 3), or the sequence's element shape."""
    if isinstance(per_sample, (list, tuple)):
        values = [np.asarray(v, dtype=np.float32) for v in per_sample]
    else:
        a = np.asarray(per_sample, dtype=np.float32)
        n, k = a.shape[0], a.shape[1]
        g = max(1, int(rays_per_output))
        assert n % g == 0
        a = a.reshape(n // g, g * k, 3)
        values = [a[:, i] for i in range(g * k)]
    acc = np.zeros_like(values[0], dtype=np.float32)
    for v in values:
        acc = (acc + v).astype(np.float32)
    return (acc / np.float32(len(values))).astype(np.float32)


def tonemap(fb):
    fb = np.ascontiguousarray(fb, dtype=np.float32)
    out = np.zeros(fb.shape, dtype=np.uint8)
    lib().rto_tonemap_rgb8(_abi.fptr(fb), fb.size // 3, _abi.u8ptr(out))
    return out


def minstd_sequence(seed, n):
    out = np.zeros(n, dtype=np.float32)
    lib().rto_minstd_sequence(seed, n, _abi.fptr(out))
    return out


def minstd_below_sequence(seed, bound, n):
    out = np.zeros(n, dtype=np.uint32)
    lib().rto_minstd_below_sequence(seed, bound, n, _abi.u32ptr(out))
    return out


def bg_uv(dirs, restated):
    """Scene::bg_at's texture coordinates for directions (n, 3): through libm as the oracle's render loop computes them, or through the
    restatement the device evaluates (include/rt_devspec.h rt_bg_uv)."""
    dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((dirs.shape[0], 2), dtype=np.float32)
    lib().rto_bg_uv(_abi.fptr(dirs), dirs.shape[0], int(bool(restated)), _abi.fptr(out))
    return out


def sincos(phi, libm=False):
    """(sin, cos) of float32 angles: the restatement the device evaluates (include/rt_devspec.h rt_sincos_libm), or with libm=True the
    host libm's sinf / cosf, which is what the oracle's render loop calls."""
    phi = np.ascontiguousarray(phi, dtype=np.float32)
    s = np.zeros_like(phi)
    c = np.zeros_like(phi)
    (lib().rto_libm_sincos if libm else lib().rto_sincos)(_abi.fptr(phi), phi.size, _abi.fptr(s), _abi.fptr(c))
    return s, c


def xoshiro_raw(state, n):
    st = np.ascontiguousarray(state, dtype=np.uint32)
    out = np.zeros(n, dtype=np.uint32)
    lib().rto_xoshiro_raw(_abi.u32ptr(st), n, _abi.u32ptr(out))
    return out


def xoshiro_below_sequence(seed, pixel, sample, bound, n):
    out = np.zeros(n, dtype=np.uint32)
    lib().rto_xoshiro_below_sequence(seed, pixel, sample, bound, n, _abi.u32ptr(out))
    return out


def xoshiro_sequence(seed, pixel, sample, n):
    out = np.zeros(n, dtype=np.float32)
    lib().rto_xoshiro_sequence(seed, pixel, sample, n, _abi.fptr(out))
    return out


def read_ppm(path):
    with open(path, "rb") as f:
        data = f.read()
    assert data[:2] == b"P6"
    parts = data.split(b"\n", 3)
    w, h = (int(x) for x in parts[1].split())
    assert parts[2] == b"255"
    return np.frombuffer(parts[3], dtype=np.uint8).reshape(h, w, 3)


# ----------------------------------------------------------------------------- reference binary (container only)
def run_reference(gltf_path, width, height, samples, out_ppm):
    """Run the UNMODIFIED reference binary (oracle/_ref/raytracer_ref). Only where it has been built."""
    subprocess.check_call([REF_BINARY, gltf_path, str(width), str(height), str(samples), out_ppm], stdout=subprocess.DEVNULL)
    return read_ppm(out_ppm)


def ref_probe(mode, gltf_path, width, height, *args):
    subprocess.check_call([REF_PROBE, mode, gltf_path, str(width), str(height), *[str(a) for a in args]], stdout=subprocess.DEVNULL)
