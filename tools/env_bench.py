#!/usr/bin/env python3
"""tools/env_bench.py — what a float environment costs in wf_shade (DESIGN.md "Environment lighting"): appends to profiles/env_importance.txt.

The sponza-like scene of bench.make_scene at --size x --size x --spp under a --sky-width x --sky-width/2 sky with a small sun, rendered
--repeat times each as (a) the 8-bit map of rt_create (bg_texture: the sky clipped and quantised), (b) the float map of rt_set_environment
without RT_ENV_IMPORTANCE, (c) with it. Prints the device time of each call (rt_stats.kernel_ms) and the time rt_set_environment took.
The three variants launch three different wf_shade instantiations (environment kind 1, 2, 3), so a kernel trace of this process
(rocprofv3 --kernel-trace --stats -- python tools/env_bench.py) splits wf_shade's time per launch by variant on its own.
Every GPU step runs under --step-timeout: a step that outlives it ends the process (status 124); nothing is retried."""
import argparse, importlib, os, statistics, sys, threading, time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1000)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--sky-width", type=int, default=2048)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--step-timeout", type=float, default=120.0)
ap.add_argument("--out", default=None, help="default: profiles/env_importance.txt of this checkout")
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = args.out or os.path.join(HERE, "profiles", "env_importance.txt")
sys.path.insert(0, HERE)
import torch  # noqa: E402,F401  (before the library: bench.py's rule)
import bench  # noqa: E402

rt = importlib.import_module("raytracing-course-hw-public_amd")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def step(what, fn):
    def expired():
        sys.stderr.write(f"env_bench: step '{what}' exceeded {args.step_timeout:.0f} s\n")
        sys.stderr.flush()
        os._exit(124)

    t = threading.Timer(args.step_timeout, expired)
    t.daemon = True
    t.start()
    try:
        return fn()
    finally:
        t.cancel()


def make_sky(w, h):
    v = (np.arange(h) + 0.5)[:, None] / h
    u = (np.arange(w) + 0.5)[None, :] / w
    base = 0.05 + 0.6 * np.clip(1.0 - 1.6 * v, 0.0, 1.0) + 0.0 * u
    sky = np.stack([0.55 * base, 0.75 * base, 1.0 * base], axis=2)
    sun = ((u - 0.62) * 2.0) ** 2 + (v - 0.22) ** 2 < (4.0 / h) ** 2  # a disc a few texels across
    sky[sun] = (3000.0, 2700.0, 2100.0)
    return sky.astype(np.float32)


wl = bench.WORKLOADS["sponza"]
W = H = args.size
sky = make_sky(args.sky_width, args.sky_width // 2)
ldr = np.empty(sky.shape[:2] + (4,), dtype=np.uint8)
ldr[..., :3] = np.round(np.clip(sky, 0.0, 1.0) ** (1.0 / 2.2) * 255.0).astype(np.uint8)
ldr[..., 3] = 255
sc = bench.make_scene(rt, wl, wl["triangles"], wl["tex_size"], W / H)
with_tex = bench.make_scene(rt, wl, wl["triangles"], wl["tex_size"], W / H)
with_tex.textures = list(with_tex.textures) + [ldr]
with_tex.bg_texture = len(with_tex.textures) - 1

say(f"# tools/env_bench.py  kernel_src_sha16 {bench.kernel_source_hash()}  library {rt.lib().rt_source_stamp().decode()}  {wl['label']} {W}x{H}x{args.spp}, "
    f"parity traversal, sky {sky.shape[1]}x{sky.shape[0]} with a sun of 3000, {args.repeat} renders each after one warm-up; device ms per render (rt_stats.kernel_ms)")
results = {}
for name, scene, env in (("8-bit map (bg_texture, wf_shade kind 1)", with_tex, None), ("float map (wf_shade kind 2)", sc, False),
                         ("float map + RT_ENV_IMPORTANCE (wf_shade kind 3)", sc, True)):
    dev = step("rt_create", lambda: rt.DeviceScene(scene))
    if env is not None:
        t0 = time.perf_counter()
        step("rt_set_environment", lambda: dev.set_environment(sky, importance=env))
        say(f"  rt_set_environment ({'with' if env else 'without'} the tables): {(time.perf_counter() - t0) * 1e3:.1f} ms wall")
    step(f"warm-up {name}", lambda: dev.run_raytracer(W, H, args.spp, seed=1))
    ms = [step(f"{name} {i}", lambda: dev.run_raytracer(W, H, args.spp, seed=1)[1]["kernel_ms"]) for i in range(args.repeat)]
    results[name] = statistics.median(ms)
    say(f"  {name:50s} median {statistics.median(ms):8.2f} ms   runs: {' '.join(f'{x:.2f}' for x in ms)}")
    dev.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n")
