#!/usr/bin/env python3
"""tools/flow_bench.py — what the motion-vector layer of an accumulator costs (DESIGN.md "Motion vectors"): writes profiles/flow.txt.

S-sponza of bench.make_scene as an 8-wide tree built on the device, 1000 x 1000, 64 samples per call. Key 1 displaces every vertex a
little and the second view is moved and turned, so every hit gathers both keys and projects twice. In one process, in alternating pairs
(plain, flow, plain, flow, ...), so that every comparison is between neighbours in time:
  * render(64) of a plain accumulator and of one with flow attached: the layer's cost on a call;
  * the same pair with RT_ACCUM_FEATURES on both sides: the cost beside the layer it resembles most.
With --profile-run the tool renders one call of a feature accumulator with flow and nothing else: run it under
`rocprofv3 --kernel-trace --stats` to read the device time of wf_flow beside wf_features of the same passes (profiles/flow.txt quotes it).
Every figure is the median of --repeat rounds, with the spread (min .. max) beside it."""
import argparse, dataclasses, importlib, os, statistics, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--triangles", type=int, default=0, help="default: the workload's (a smaller count is a rehearsal, not a measurement)")
ap.add_argument("--tex-size", type=int, default=-1)
ap.add_argument("--size", type=int, default=0, help="image width = height (default: the workload's 1000)")
ap.add_argument("--out", default=None, help="default: profiles/flow.txt of this checkout")
ap.add_argument("--profile-run", action="store_true", help="one render(64) of a feature accumulator with flow, for a kernel trace; writes no file")
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import numpy as np
import torch  # noqa: F401  (before the library: bench.py's rule)
import bench

rt = importlib.import_module("raytracing-course-hw-public_amd")
out_path = args.out or os.path.join(HERE, "profiles", "flow.txt")
lines = []
SPP = 64


def say(s):
    print(s, flush=True)
    lines.append(s)


def fmt(ts):
    return f"{statistics.median(ts):9.2f} ms (min {min(ts):8.2f} .. max {max(ts):8.2f}, n = {len(ts)})"


wl = bench.WORKLOADS["sponza"]
n_tri = args.triangles or wl["triangles"]
W = H = args.size or wl["width"]
sc0 = bench.make_scene(rt, wl, n_tri, wl["tex_size"] if args.tex_size < 0 else args.tex_size, 1.0)
p0 = np.asarray(sc0.positions, dtype=np.float32)
sc1 = dataclasses.replace(sc0, positions=(p0 + np.random.default_rng(1).normal(scale=0.05, size=p0.shape).astype(np.float32)).astype(np.float32))
cam0 = sc0.camera
cam1 = dataclasses.replace(rt.scenegen.look_camera(np.asarray(cam0.position, dtype=np.float32) + np.array([0.5, 0.1, -0.3], dtype=np.float32), yaw_deg=-88.0, yfov=0.9), fov_x=cam0.fov_x)
s0, s1 = rt.Sensor.pinhole(cam0, seed=1), rt.Sensor.pinhole(cam1, seed=2)
dev = rt.DeviceScene(sc0, wide=True, device_bvh=True)
flow = dict(key0=sc0, key1=sc1, sensor1=s1)


def render(**kw):
    acc = dev.accumulator(W, H, sensor=s0, **kw)
    t0 = time.perf_counter()
    st = acc.render(SPP)  # returns with the scene's stream synchronised
    ms = (time.perf_counter() - t0) * 1e3
    valid = float(acc.flow()[1].mean()) if "flow" in kw else None
    acc.close()
    return ms, st["kernel_ms"], valid


if args.profile_run:
    ms, kernel_ms, valid = render(features=True, flow=flow)
    print(f"profile run: render({SPP}) {ms:.2f} ms wall, {kernel_ms:.2f} ms on the device; mean mask {valid:.4f}")
    dev.close()
    sys.exit(0)

say(f"# tools/flow_bench.py  kernel_src_sha16 {bench.kernel_source_hash()}  library {rt.lib().rt_source_stamp().decode()}")
say(f"# {wl['label']}, {sc0.n_triangles} triangles, wide + device-built, {W} x {H}, render({SPP}); key 1 displaces every vertex, the second view is moved and turned;")
say(f"# alternating pairs in one process, median of {args.repeat} rounds (one warm-up round dropped); keys as two arrays of 36 B per triangle")
VARIANTS = [("plain", {}), ("flow", dict(flow=flow)), ("features", dict(features=True)), ("features + flow", dict(features=True, flow=flow))]
res = {name: [] for name, _ in VARIANTS}
mask = None
for rnd in range(args.repeat + 1):
    for name, kw in VARIANTS:
        ms, kernel_ms, valid = render(**kw)
        mask = valid if valid is not None else mask
        if rnd:
            res[name].append((ms, kernel_ms))
dev.close()
for name, _ in VARIANTS:
    say(f"{name:16s} wall {fmt([r[0] for r in res[name]])}   device {fmt([r[1] for r in res[name]])}")
med = {name: statistics.median(r[1] for r in res[name]) for name in res}
say(f"flow on a plain accumulator:   {med['flow'] - med['plain']:+8.2f} ms of device time per call = {med['flow'] / med['plain']:.4f} x")
say(f"flow on a feature accumulator: {med['features + flow'] - med['features']:+8.2f} ms of device time per call = {med['features + flow'] / med['features']:.4f} x")
say(f"mean mask of the flow (share of samples with a flow): {mask:.4f}")
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
