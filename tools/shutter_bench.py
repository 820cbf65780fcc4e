#!/usr/bin/env python3
"""tools/shutter_bench.py — what a shutter accumulator's slice change costs (DESIGN.md "Shutter"): writes profiles/shutter.txt.

S-sponza of bench.make_scene as an 8-wide tree built on the device, 1000 x 1000, 64 samples. Key 1 moves a tenth of the triangles (a block
of the random ones) by a tenth of the room; in the "moving lights" variant one emissive triangle moves too. In one process, alternating, so
that every comparison is between neighbours in time:
  * the parent's capability: rt_update_geometry_device(RT_UPDATE_REFIT) over arrays that were blended beforehand and are in HBM, wall time
    per call (two frames alternate, so no call updates to what the scene already holds);
  * a plain accumulator's render(64), and the same 64 samples as 16 calls of 4 and as 64 calls of 1: what cutting a call into runs costs by
    itself (a plan, a read-back and the launch tails of ray_depth bounces per run), without any slice change;
  * shutter accumulators with (K, B) = (16, 4) and (64, 1), moving lights and static lights: the wall time of render(64) and, from
    rt_accum_shutter_times, the wall time per slice change.
Expectation, stated before the first run: a slice change does the parent call's device work plus one streaming blend and skips its pointer
checks, so with moving lights it should stay within 10 % of that call; with static lights it should be clearly faster, because the light
list, the host light build and the tree's way back go away. The last lines say whether that held.
Every figure is the median of --repeat rounds, with the spread (min .. max) beside it."""
import argparse, ctypes as C, dataclasses, importlib, os, statistics, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--triangles", type=int, default=0, help="default: the workload's (a smaller count is a rehearsal, not a measurement)")
ap.add_argument("--tex-size", type=int, default=-1)
ap.add_argument("--size", type=int, default=0, help="image width = height (default: the workload's 1000)")
ap.add_argument("--out", default=None, help="default: profiles/shutter.txt of this checkout")
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))
import numpy as np
import torch  # noqa: F401  (before the library: bench.py's rule)
import bench
import shutter_replay as R

rt = importlib.import_module("raytracing-course-hw-public_amd")
out_path = args.out or os.path.join(HERE, "profiles", "shutter.txt")
lines = []
SPP = 64


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    t0 = time.perf_counter()
    fn()  # every entry point returns with the scene's stream synchronised
    return (time.perf_counter() - t0) * 1e3


def fmt(ts):
    return f"{statistics.median(ts):9.2f} ms (min {min(ts):8.2f} .. max {max(ts):8.2f}, n = {len(ts)})"


wl = bench.WORKLOADS["sponza"]
n_tri = args.triangles or wl["triangles"]
W = H = args.size or wl["width"]
sc0 = bench.make_scene(rt, wl, n_tri, wl["tex_size"] if args.tex_size < 0 else args.tex_size, 1.0)
FIRST = 12 + 16  # walls and lights come first (scenegen.room_scene)
block = slice(FIRST + n_tri // 2, FIRST + n_tri // 2 + n_tri // 10)
p1 = np.asarray(sc0.positions, dtype=np.float32).copy()
p1[block] += np.array([4.0, 1.0, -2.0], dtype=np.float32)
static = dataclasses.replace(sc0, positions=p1)
p2 = p1.copy()
p2[12] += np.array([2.0, -0.5, 1.0], dtype=np.float32)
moving = dataclasses.replace(sc0, positions=p2)
key0 = rt.geometry_arrays(sc0)
say(f"# tools/shutter_bench.py  kernel_src_sha16 {bench.kernel_source_hash()}  library {rt.lib().rt_source_stamp().decode()}")
say(f"# {wl['label']}, {len(key0['material_ids'])} triangles, wide + device-built, {W} x {H}, {SPP} samples; key 1 moves {n_tri // 10} triangles; median of {args.repeat} rounds")

dev = rt.DeviceScene(sc0, wide=True, device_bvh=True)


# ---- the parent's capability: pre-blended arrays in HBM, rt_update_geometry_device(REFIT)
def device_frame(key1, t):
    arrays = R.geometry_at(key0, key1, t)
    tens = {k: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0") for k, a in arrays.items()}
    u = rt.RtGeometryUpdate()
    u.n_triangles = arrays["material_ids"].size
    u.mode = rt.RT_UPDATE_REFIT
    for k, v in tens.items():
        setattr(u, k, C.cast(C.c_void_p(v.data_ptr()), type(getattr(u, k))))
    return u, tens


key1_moving = rt.geometry_arrays(moving)
frames = [device_frame(key1_moving, R.slice_time(k, 16)) for k in (3, 12)]
torch.cuda.synchronize()
turn = [0]


def parent_update():
    u = frames[turn[0] % 2][0]
    turn[0] += 1
    rc = rt.lib().rt_update_geometry_device(dev._h, C.byref(u))
    assert rc == 0, rt.lib().rt_last_error().decode()


def plain_render(calls=1):
    acc = dev.accumulator(W, H, seed=1)
    t = timed(lambda: [acc.render(SPP // calls) for _ in range(calls)])
    acc.close()
    return t


def shutter_render(key1, K, B):
    acc = dev.accumulator(W, H, seed=1, shutter=dict(key0=sc0, key1=key1, slices=K, block=B, refit=True))
    t = timed(lambda: acc.render(SPP))
    times, info = acc.shutter_times(), acc.shutter_info()
    acc.close()
    return t, times["slice_change_ms"] / times["slice_changes"], times["slice_changes"], info


VARIANTS = [("moving lights", moving, 16, 4), ("static lights", static, 16, 4), ("moving lights", moving, 64, 1), ("static lights", static, 64, 1)]
res = {"parent": [], "plain": [], "plain16": [], "plain64": [], **{(name, K, B): [] for name, _, K, B in VARIANTS}}
for rnd in range(args.repeat + 1):  # round 0 warms every shape up and is dropped
    got = {"parent": [timed(parent_update) for _ in range(4)], "plain": [plain_render()], "plain16": [plain_render(16)], "plain64": [plain_render(64)]}
    for name, key1, K, B in VARIANTS:
        got[(name, K, B)] = [shutter_render(key1, K, B)]
    if rnd:
        for k, v in got.items():
            res[k] += v
dev.close()

parent = statistics.median(res["parent"])
plain = statistics.median(res["plain"])
say(f"rt_update_geometry_device(REFIT), pre-blended arrays in HBM (the parent's slice change): {fmt(res['parent'])}")
say(f"plain accumulator, render({SPP}):                                                     {fmt(res['plain'])}")
say(f"plain accumulator, the same samples as 16 x render(4):                                {fmt(res['plain16'])}")
say(f"plain accumulator, the same samples as 64 x render(1):                                {fmt(res['plain64'])}")
split = {16: statistics.median(res["plain16"]), 64: statistics.median(res["plain64"])}
per_slice = {}
for name, key1, K, B in VARIANTS:
    r = res[(name, K, B)]
    call, change = [x[0] for x in r], [x[1] for x in r]
    per_slice[(name, K, B)] = statistics.median(change)
    say(f"shutter K = {K:2d}, B = {B}, {name}: render({SPP}) {fmt(call)} = {statistics.median(call) / plain:5.2f} x plain, {statistics.median(call) / split[K]:5.2f} x plain in {K} calls; {r[0][2]} slice changes, "
        f"per change {fmt(change)} = {statistics.median(change) / parent:5.2f} x the parent call; static_lights = {r[0][3]['static_lights']}")
mv, stc = per_slice[("moving lights", 16, 4)], per_slice[("static lights", 16, 4)]
say(f"expectation 1 (moving lights: a slice change within 10 % of the parent call): {'confirmed' if mv <= 1.10 * parent else 'NOT confirmed'}: {mv:.2f} ms against {parent:.2f} ms")
say(f"expectation 2 (static lights: clearly faster than the parent call): {'confirmed' if stc < 0.9 * parent else 'NOT confirmed'}: {stc:.2f} ms against {parent:.2f} ms"
    f" (what it skips is the light half of a moving-lights change, {mv - stc:.2f} ms for this scene's 16 emissive triangles)")
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
