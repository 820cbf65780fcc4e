#!/usr/bin/env python3
"""tools/id_mattes_cost.py — what id mattes cost an accumulator (include/rt_abi.h rt_accum_attach_ids; DESIGN.md "Id mattes"): acc.render(8)
at 1000 x 1000 on the S-sponza scene of bench.make_scene, in the parity build and the production build (device + wide, global-best
traversal), for an accumulator without ids, with ids (MATERIAL, K = 4; PRIMITIVE, K = 16) and, for scale, with the first-hit feature sums.
Every variant renders on a fresh accumulator; the variants alternate within each of the rounds, and the medians of kernel_ms (the device span
of the call) are compared. Also times the three reads. Appends nothing: redirect the output to profiles/id_mattes.txt."""
import importlib, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401
import bench
rt = importlib.import_module("raytracing-course-hw-public_amd")
W = H = 1000
SPP, ROUNDS, SEED = 8, 7, 7
wl = bench.WORKLOADS["sponza"]
sc = bench.make_scene(rt, wl, wl["triangles"], wl["tex_size"], W / H)
print(f"# tools/id_mattes_cost.py on one MI355X: S-sponza {W}x{H}, acc.render({SPP}) on a fresh accumulator, median of {ROUNDS} alternating rounds after one warm-up round")
print(f"kernel_src_sha16 {bench.kernel_source_hash()}  library {rt.lib().rt_source_stamp().decode()}")
VARIANTS = (("no ids", {}), ("ids material K=4", dict(ids="material", id_slots=4)), ("ids primitive K=16", dict(ids="primitive", id_slots=16)),
            ("features", dict(features=True)), ("features + ids material K=4", dict(features=True, ids="material", id_slots=4)))

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
    base = statistics.median(ms["no ids"])
    for v, _ in VARIANTS:
        m = statistics.median(ms[v])
        print(f"{name:10s} {v:28s}: kernel_ms median {m:8.3f}  (min {min(ms[v]):8.3f}, max {max(ms[v]):8.3f})  {100.0 * (m - base) / base:+6.2f} % of the plain render")
    acc = dev.accumulator(W, H, seed=SEED, ids="material", id_slots=4)
    acc.render(SPP, global_best=gb)
    other = acc.read_ids()["other"]
    print(f"{name:10s} material K=4: pixels with other > 0: {int(np.count_nonzero(other))} of {other.size}")

    def best(fn, n=10):
        fn()
        out = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return min(out)

    print(f"{name:10s} reads (host outputs, wall ms, best of 10): labels {best(acc.labels):.3f}  matte of 3 ids {best(lambda: acc.matte([0, 1, 2])):.3f}  "
          f"read_ids {best(acc.read_ids):.3f}")
    acc.close()
    dev.close()
