#!/usr/bin/env python3
"""tools/light_groups_cost.py — what light groups cost an accumulator (include/rt_abi.h rt_accum_attach_light_groups; DESIGN.md "Light groups"):
acc.render(8) at 1000 x 1000 on the S-sponza scene of bench.make_scene, in the parity build and the production build (device + wide,
global-best traversal), for an accumulator without groups, with G = 1, 4 and 8 groups and, for scale, with the first-hit feature sums. With
G groups material m is in group m % max(G - 1, 1) and the background in group G - 1: every hit and every miss has a group, as the tag kernel
pays the same for an emitter as for any other material. Every variant renders on a fresh accumulator; the variants alternate within each of
the rounds, and the medians of kernel_ms (the device span of the call) are compared. Also times light_mix into a device buffer and
read_light_groups. Appends nothing: redirect the output to profiles/light_groups.txt."""
import importlib, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench
rt = importlib.import_module("raytracing-course-hw-public_amd")
W = H = 1000
SPP, ROUNDS, SEED = 8, 7, 7
wl = bench.WORKLOADS["sponza"]
sc = bench.make_scene(rt, wl, wl["triangles"], wl["tex_size"], W / H)
n_mat = len(sc.materials)
print(f"# tools/light_groups_cost.py on one MI355X: S-sponza {W}x{H} ({n_mat} materials), acc.render({SPP}) on a fresh accumulator, median of {ROUNDS} alternating rounds after one warm-up round")
print(f"kernel_src_sha16 {bench.kernel_source_hash()}  library {rt.lib().rt_source_stamp().decode()}")


def groups(G):
    return dict(light_groups=dict(material_group=[m % max(G - 1, 1) for m in range(n_mat)], background=G - 1, n_groups=G))


VARIANTS = (("no groups", {}), ("G = 1", groups(1)), ("G = 4", groups(4)), ("G = 8", groups(8)), ("features", dict(features=True)),
            ("features + G = 8", dict(features=True, **groups(8))))

for name, kw, gb in (("parity", {}, False), ("production", dict(device_bvh=True, wide=True), True)):
    dev = rt.DeviceScene(sc, **kw)
    ms = {v: [] for v, _ in VARIANTS}
    for r in range(ROUNDS + 1):
        for v, akw in VARIANTS:
            acc = dev.accumulator(W, H, seed=SEED, **akw)
            st = acc.render(SPP, global_best=gb)
            if r > 0:
                ms[v].append(st["kernel_ms"])
            acc.close()
    base = statistics.median(ms["no groups"])
    for v, _ in VARIANTS:
        m = statistics.median(ms[v])
        print(f"{name:10s} {v:18s}: kernel_ms median {m:8.3f}  (min {min(ms[v]):8.3f}, max {max(ms[v]):8.3f})  {100.0 * (m - base) / base:+6.2f} % of the plain render")
    acc = dev.accumulator(W, H, seed=SEED, **groups(8))
    acc.render(SPP, global_best=gb)
    out = torch.zeros((H, W, 3), dtype=torch.float32, device=f"cuda:{dev._device}")
    torch.cuda.synchronize()
    wts = np.linspace(0.25, 2.0, 24, dtype=np.float32).reshape(8, 3)

    def best(fn, n=10):
        fn()
        t = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return min(t)

    GS = acc.read_light_groups()
    S = acc.read()["sum"]
    rel = np.abs(GS.sum(axis=0, dtype=np.float64) - S) / np.maximum(np.abs(S), 1e-6)
    print(f"{name:10s} G = 8: max relative |sum of the group sums - S| = {rel.max():.3e} (float addition is not associative)")
    print(f"{name:10s} G = 8 reads (wall ms, best of 10): light_mix to a device buffer {best(lambda: acc.light_mix(wts, device_out=out.data_ptr())):.3f}  "
          f"light_mix rgb8 to a device buffer {best(lambda: acc.light_mix(wts, rgb8=True, device_out=out.data_ptr())):.3f}  "
          f"light_group to the host {best(lambda: acc.light_group(3)):.3f}  read_light_groups {best(acc.read_light_groups):.3f}")
    acc.close()
    dev.close()
