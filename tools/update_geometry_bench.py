#!/usr/bin/env python3
"""tools/update_geometry_bench.py — what rt_update_geometry saves and what a refit gives up (DESIGN.md "Geometry updates"): writes
profiles/update_geometry.txt.

On the scenes of bench.make_scene (S-sponza, S-10M), for each build kind (reference, reference+wide, device, device+wide), with a wave
deformation of the scene as the new geometry (0.05 L per vertex, shared vertices stay shared):
  * wall time of rt_destroy + rt_create of the new geometry (what a caller does without the entry point);
  * wall time of RT_UPDATE_REBUILD, and of RT_UPDATE_REFIT on the wide kinds;
  * nodes_visited per cast (RT_FLAG_COUNTERS) and Msamples/s at 16 SPP on the refitted tree and on the rebuilt tree of the same geometry.
--tree DIR runs the first item on another checkout of the project (one built from the parent commit has no rt_update_geometry: only
rt_destroy + rt_create is timed there). Every figure is the best of --repeat runs; the deformations alternate, so no run updates to what
the scene already holds."""
import argparse, dataclasses, importlib, os, sys, time

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
has_update = hasattr(rt.DeviceScene, "update_geometry")
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
    for kind in args.kinds.split(","):
        kw = KINDS[kind]
        state = {"dev": rt.DeviceScene(sc, **kw), "i": 0}

        def recreate():
            state["dev"].close()
            state["dev"] = rt.DeviceScene(frames[state["i"] % 2], **kw)
            state["i"] += 1

        def update(refit):
            state["dev"].update_geometry(frames[state["i"] % 2], refit=refit)
            state["i"] += 1

        t_create = best(recreate, args.repeat)
        say(f"{wl['label']:9s} {kind:15s} rt_destroy + rt_create of the new geometry: {t_create:9.1f} ms wall")
        if has_update:
            t_rebuild = best(lambda: update(False), args.repeat)
            state["i"] = 0
            update(False)  # both trees are judged on frames[0]
            nv, ms = quality(state["dev"], W, H)
            say(f"{wl['label']:9s} {kind:15s} RT_UPDATE_REBUILD:                          {t_rebuild:9.1f} ms wall   rebuilt tree:   {nv:7.2f} nodes_visited / cast, {ms:8.1f} Msamples/s at 16 SPP")
            if kw.get("wide"):
                state["dev"].close()
                state["dev"] = rt.DeviceScene(sc, **kw)  # the topology of the undeformed scene, refitted to the wave
                state["i"] = 0
                t_refit = best(lambda: update(True), args.repeat)
                state["i"] = 0
                update(True)
                nv, ms = quality(state["dev"], W, H)
                say(f"{wl['label']:9s} {kind:15s} RT_UPDATE_REFIT:                            {t_refit:9.1f} ms wall   refitted tree:  {nv:7.2f} nodes_visited / cast, {ms:8.1f} Msamples/s at 16 SPP")
        state["dev"].close()
with open(out_path, "a" if args.tree or args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
