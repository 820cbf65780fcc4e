#!/usr/bin/env python3
"""tools/adaptive_timing.py — uniform against adaptive sampling through the accumulators (include/rt_abi.h rt_accum_*; DESIGN §6, "Adaptive against uniform sampling") on the
S-sponza scene of bench.make_scene at 1000 x 1000, in the parity build and the production build (device + wide, global-best traversal).

  * reference: 1024 SPP built progressively through one accumulator (8 calls of 128 samples), with ANOTHER seed than the images it judges:
               with the same seed its first 256 samples would be theirs and the RMSE would shrink with the samples they share
  * uniform:   rt_render at 16, 32, 64, 128, 256 SPP: wall ms and RMSE against the reference
  * adaptive:  min 16, max 256 at three thresholds (the 80th, 90th and 97th percentile of err after 16 samples; below the 50th the 3x3
               window sends nearly every pixel to the cap), each with step 16, 32 and 64: wall ms, mean SPP, rounds, RMSE, and the RMSE
               of the uniform render of equal wall time (interpolated)
  * overhead:  one judge + scan + read-back with nothing left to add (an adaptive call on an accumulator that has converged), and the floor
               of a small round: an accumulator of N pixels given `step` samples (N x step paths in one pass)
Heavy runs are single runs after one warm-up; the overhead rows are the best of 20."""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401
import bench
rt = importlib.import_module("raytracing-course-hw-public_amd")
W = H = 1000
SEED, REF_SEED = 7, 1007
wl = bench.WORKLOADS["sponza"]
sc = bench.make_scene(rt, wl, wl["triangles"], wl["tex_size"], W / H)
print(f"# tools/adaptive_timing.py on one MI355X: S-sponza {W}x{H}, seed {SEED}")
print(f"kernel_src_sha16 {bench.kernel_source_hash()}  library {rt.lib().rt_source_stamp().decode()}")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def best(fn, n=20):
    fn()
    return min(timed(fn)[0] for _ in range(n))


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


for name, kw, gb in (("parity", {}, False), ("production", dict(device_bvh=True, wide=True), True)):
    dev = rt.DeviceScene(sc, **kw)
    ref_acc = dev.accumulator(W, H, seed=REF_SEED)
    t_ref = 0.0
    for _ in range(8):
        t, _ = timed(lambda: ref_acc.render(128, global_best=gb))
        t_ref += t
    ref = ref_acc.image()
    ref_acc.close()
    print(f"\n== {name}: reference 1024 SPP (seed {REF_SEED}) through the accumulator in 8 x 128: {t_ref:.0f} ms")
    dev.run_raytracer(W, H, 16, seed=SEED, global_best=gb)  # warm-up
    uniform = []
    for spp in (16, 32, 64, 128, 256):
        t, (fb, _) = timed(lambda: dev.run_raytracer(W, H, spp, seed=SEED, global_best=gb))
        uniform.append((spp, t, rmse(fb, ref)))
        print(f"{name:10s} uniform  rt_render {spp:4d} SPP: wall {t:8.1f} ms  RMSE {uniform[-1][2]:.5f}")
    probe = dev.accumulator(W, H, seed=SEED)
    probe.render_adaptive(3.0e38, min_samples=16, max_samples=16, step=16, global_best=gb)
    err = probe.read()["error"]
    probe.close()
    fin = err[np.isfinite(err)]
    print(f"{name:10s} err after 16 SPP: percentiles 20/50/80/90/97 = " + " / ".join(f"{np.quantile(fin, q):.4g}" for q in (0.2, 0.5, 0.8, 0.9, 0.97)))
    thresholds = [float(np.float32(np.quantile(fin, q))) for q in (0.8, 0.9, 0.97)]

    def adaptive(thr, step, quiet=False):
        acc = dev.accumulator(W, H, seed=SEED)
        t, st = timed(lambda: acc.render_adaptive(thr, min_samples=16, max_samples=256, step=step, global_best=gb))
        n = acc.read()["samples"]
        e = rmse(acc.image(), ref)
        acc.close()
        # the uniform render of equal wall time, interpolated on the rows above (log SPP vs log RMSE is near linear)
        ts, es = np.array([u[1] for u in uniform]), np.array([u[2] for u in uniform])
        e_eq = float(np.exp(np.interp(t, ts, np.log(es)))) if ts[0] <= t <= ts[-1] else float("nan")
        if not quiet:
            print(f"{name:10s} adaptive thr {thr:9.4g} step {step:3d}: wall {t:8.1f} ms  mean SPP {n.mean():7.2f}  rounds {st['rounds']:3d}  "
                  f"passes {st['passes']:3d}  RMSE {e:.5f}  | uniform at equal wall (interpolated) RMSE {e_eq:.5f}")

    adaptive(thresholds[0], 16, quiet=True)  # warm-up of the round machinery at this size
    for thr in thresholds:
        for step in (16, 32, 64):
            adaptive(thr, step)
    # overhead of one judge with nothing to add: round 0 (nothing below min) + the judge that ends the call
    conv = dev.accumulator(W, H, seed=SEED)
    conv.render(16, global_best=gb)
    t = best(lambda: conv.render_adaptive(3.0e38, min_samples=16, max_samples=256, step=16, global_best=gb))
    k = min(conv.render_adaptive(3.0e38, min_samples=16, max_samples=256, step=16, global_best=gb)["kernel_ms"] for _ in range(20))
    print(f"{name:10s} overhead: adaptive call with nothing to add (2 x (target + plan scan + 8-byte read-back), 1 x err): wall {t:.3f} ms, device span {k:.3f} ms")
    conv.close()
    for n_pix in (1000, 10000, 100000):
        for step in (16, 32, 64):
            small = dev.accumulator(n_pix // 100, 100, seed=SEED)
            t = best(lambda: small.render(step, global_best=gb), n=5)
            small.close()
            print(f"{name:10s} small round: {n_pix:6d} pixels x {step:3d} samples ({n_pix * step:8d} paths, one pass): wall {t:7.2f} ms")
    dev.close()
