#!/usr/bin/env python3
"""tools/update_geometry_bench.py — what rt_update_geometry saves and what a refit gives up (DESIGN.md "Geometry updates"): writes
profiles/update_geometry.txt.

On the scenes of bench.make_scene (S-sponza, S-10M), for each build kind (reference, reference+wide, device, device+wide), with a wave
deformation of the scene as the new geometry (0.05 L per vertex, shared vertices stay shared):
  * wall time of rt_destroy + rt_create of the new geometry (what a caller does without the entry point);
  * wall time of RT_UPDATE_REBUILD, and of RT_UPDATE_REFIT on the wide kinds, through rt_update_geometry (host arrays) and through
    rt_update_geometry_device (the same bytes as torch tensors that are in HBM before the timer starts). Both legs start from equally
    prepared data: rt.geometry_arrays flattens each frame once, the rt_geometry_update structs are filled before the timer, and the timer
    holds the library call alone (no descriptor building, no normal generation, no numpy copy on either side);
  * for REFIT, rt_refit_times: the refit on the device and the share of it and of the call spent in the top-down level pass (k_refit_level and
    its one host read per level), which depends on the topology alone and could be cached on the scene;
  * nodes_visited per cast (RT_FLAG_COUNTERS) and Msamples/s at 16 SPP on the refitted tree and on the rebuilt tree of the same geometry.
--tree DIR runs the first item on another checkout of the project (one built from the parent commit has no rt_update_geometry: only
rt_destroy + rt_create is timed there). Every figure is the best of --repeat runs; the deformations alternate, so no run updates to what
the scene already holds."""
import argparse, ctypes as C, dataclasses, importlib, os, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--workloads", default="sponza,s10m")
ap.add_argument("--kinds", default="reference,reference+wide,device,device+wide")
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--tree", default=None, help="another built checkout to time rt_destroy + rt_create on")
ap.add_argument("--out", default=None, help="default: profiles/update_geometry.txt of this checkout")
ap.add_argument("--append", action="store_true", help="append to the file (always with --tree)")
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(args.tree) if args.tree else HERE
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (before the library: bench.py's rule)
import bench

rt = importlib.import_module("raytracing-course-hw-public_amd")
KINDS = {"reference": dict(), "reference+wide": dict(wide=True), "device": dict(device_bvh=True), "device+wide": dict(device_bvh=True, wide=True)}
has_update = hasattr(rt.DeviceScene, "update_geometry") and not args.tree  # --tree: only rt_destroy + rt_create is timed there
has_device = has_update and hasattr(rt.DeviceScene, "update_geometry_device")
out_path = args.out or os.path.join(HERE, "profiles", "update_geometry.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def wave(sc, amp):
    v = sc.positions.reshape(-1, 3).astype(np.float32)
    L = np.float32((v.max(axis=0) - v.min(axis=0)).max())
    d = np.stack([np.sin(np.float32(7) * v[:, 1] / L), np.sin(np.float32(5) * v[:, 2] / L), np.sin(np.float32(3) * v[:, 0] / L)], axis=1).astype(np.float32)
    return dataclasses.replace(sc, positions=(v + np.float32(amp) * L * d).astype(np.float32).reshape(-1, 3, 3))


def best(fn, n):
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return min(t) * 1e3


def update_struct(pointers, n):
    """A filled rt_geometry_update (mode is set per call) over five addresses."""
    u = rt.RtGeometryUpdate()
    u.n_triangles = n
    for k, p in pointers.items():
        setattr(u, k, C.cast(C.c_void_p(p), type(getattr(u, k))))
    return u


def prepare(sc):
    """One frame, ready for both entry points: the flat host arrays of rt.geometry_arrays, the same bytes as torch tensors on GPU 0, and a
    filled struct for each. Returns (host struct, device struct, what keeps their memory alive)."""
    arrays = rt.geometry_arrays(sc)
    n = arrays["positions"].size // 9
    host = update_struct({k: a.ctypes.data for k, a in arrays.items()}, n)
    if not has_device:
        return host, None, arrays
    t = {k: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0") for k, a in arrays.items()}
    torch.cuda.synchronize()
    return host, update_struct({k: v.data_ptr() for k, v in t.items()}, n), (arrays, t)


def call(fn, dev, u, refit):
    u.mode = rt.RT_UPDATE_REFIT if refit else rt.RT_UPDATE_REBUILD
    rc = fn(dev._h, C.byref(u))
    if rc != 0:
        raise RuntimeError(f"update failed ({rc}): {rt.lib().rt_last_error().decode()}")


def quality(dev, W, H):
    dev.run_raytracer(W, H, 16, seed=1)
    st = min((dev.run_raytracer(W, H, 16, seed=1)[1] for _ in range(3)), key=lambda s: s["kernel_ms"])
    ct = dev.run_raytracer(W, H, 1, seed=1, counters=True)[1]
    return ct["nodes_visited"] / max(1, ct["casts"]), st["samples"] / st["kernel_ms"] / 1e3


say(f"# tools/update_geometry_bench.py  tree {'parent checkout' if args.tree else 'this checkout'}  kernel_src_sha16 {bench.kernel_source_hash()}  library {rt.lib().rt_source_stamp().decode()}"
    f"  best of {args.repeat}")
for wl_name in args.workloads.split(","):
    wl = bench.WORKLOADS[wl_name]
    W, H = wl["width"], wl["height"]
    sc = bench.make_scene(rt, wl, wl["triangles"], wl["tex_size"], W / H)
    frames = [wave(sc, 0.05), wave(sc, -0.05)]  # two deformations of equal size to alternate between
    ready = [prepare(f) for f in frames] if has_update else None  # before any timer
    for kind in args.kinds.split(","):
        kw = KINDS[kind]
        state = {"dev": rt.DeviceScene(sc, **kw), "i": 0}

        def recreate():
            state["dev"].close()
            state["dev"] = rt.DeviceScene(frames[state["i"] % 2], **kw)
            state["i"] += 1

        def update(refit):
            call(rt.lib().rt_update_geometry, state["dev"], ready[state["i"] % 2][0], refit)
            state["i"] += 1

        def update_device(refit):
            call(rt.lib().rt_update_geometry_device, state["dev"], ready[state["i"] % 2][1], refit)
            state["i"] += 1

        def level_share(t_call):
            rtimes = state["dev"].refit_times()
            return (f"refit on the device {rtimes['refit_ms']:7.2f} ms, of it the level pass {rtimes['levels_ms']:7.2f} ms = "
                    f"{100 * rtimes['levels_ms'] / max(rtimes['refit_ms'], 1e-9):4.1f} % of the refit, {100 * rtimes['levels_ms'] / max(t_call, 1e-9):4.1f} % of the call's best wall time")

        t_create = best(recreate, args.repeat)
        say(f"{wl['label']:9s} {kind:15s} rt_destroy + rt_create of the new geometry: {t_create:9.1f} ms wall")
        if has_update:
            t_rebuild = best(lambda: update(False), args.repeat)
            state["i"] = 0
            update(False)  # both trees are judged on frames[0]
            nv, ms = quality(state["dev"], W, H)
            say(f"{wl['label']:9s} {kind:15s} RT_UPDATE_REBUILD:                          {t_rebuild:9.1f} ms wall   rebuilt tree:   {nv:7.2f} nodes_visited / cast, {ms:8.1f} Msamples/s at 16 SPP")
            if has_device:
                t_dev = best(lambda: update_device(False), args.repeat)
                say(f"{wl['label']:9s} {kind:15s} RT_UPDATE_REBUILD, arrays in HBM (rt_update_geometry_device): {t_dev:9.1f} ms wall   (host arrays: {t_rebuild:9.1f} ms)")
            if kw.get("wide"):
                state["dev"].close()
                state["dev"] = rt.DeviceScene(sc, **kw)  # the topology of the undeformed scene, refitted to the wave
                state["i"] = 0
                t_refit = best(lambda: update(True), args.repeat)
                state["i"] = 0
                update(True)
                share_host = level_share(t_refit) if has_device else None
                nv, ms = quality(state["dev"], W, H)
                say(f"{wl['label']:9s} {kind:15s} RT_UPDATE_REFIT:                            {t_refit:9.1f} ms wall   refitted tree:  {nv:7.2f} nodes_visited / cast, {ms:8.1f} Msamples/s at 16 SPP")
                if has_device:
                    say(f"{wl['label']:9s} {kind:15s}   last host-array REFIT:   {share_host}")
                    t_dev = best(lambda: update_device(True), args.repeat)
                    say(f"{wl['label']:9s} {kind:15s} RT_UPDATE_REFIT, arrays in HBM (rt_update_geometry_device):   {t_dev:9.1f} ms wall   (host arrays: {t_refit:9.1f} ms)")
                    say(f"{wl['label']:9s} {kind:15s}   last device-array REFIT: {level_share(t_dev)}")
        state["dev"].close()
with open(out_path, "a" if args.tree or args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
