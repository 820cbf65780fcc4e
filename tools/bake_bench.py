#!/usr/bin/env python3
"""tools/bake_bench.py — what baking on the device costs beside the two ways to bake through rt_render_rays (DESIGN.md "Baking"): writes
profiles/bake.txt.

On scenegen.room_scene(--triangles) with --points surface points (closest hits of random rays) x --spp samples, one process, for
IRRADIANCE and for SH9, --repeat interleaved rounds after one warm-up each of
  a  rt_bake, points and output in HBM;
  b  rt_bake_rays into HBM + rt_render_rays over those records, output in HBM (IRRADIANCE: K = 1, G = spp; SH9: G = 1, the per-ray values
     a caller would still have to read back and project);
  c  rt_render_rays with the same records uploaded from the host and the outputs copied back (SH9 then projects on the host: not timed).
Wall time of every call (perf_counter around the binding; each entry point returns with its stream idle), and for a the share of
rt_stats.kernel_ms outside dominant_ms (the closest-hit launches): first stage, shading, fold and resolve.
Then rt_lightmap_points on a --atlas x --atlas atlas with every triangle of the scene in its own grid cell, device arrays, wall time.
Every GPU step runs under --step-timeout (a watchdog ends the process: a hung step must not be waited for)."""
import argparse, importlib, os, statistics, sys, threading, time

ap = argparse.ArgumentParser()
ap.add_argument("--triangles", type=int, default=20000)
ap.add_argument("--points", type=int, default=1 << 18)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--atlas", type=int, default=1024)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--step-timeout", type=float, default=120.0)
ap.add_argument("--out", default=None, help="default: profiles/bake.txt of this checkout")
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
out_path = args.out or os.path.join(HERE, "profiles", "bake.txt")
lines = []

import numpy as np
import torch  # noqa: F401  (before the library: bench.py's rule)
import bench

rt = importlib.import_module("raytracing-course-hw-public_amd")


def say(s):
    print(s, flush=True)
    lines.append(s)


def step(what, fn):
    def expired():
        sys.stderr.write(f"bake_bench: step '{what}' exceeded {args.step_timeout:.0f} s\n")
        sys.stderr.flush()
        os._exit(124)

    t = threading.Timer(args.step_timeout, expired)
    t.daemon = True
    t.start()
    try:
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3
    finally:
        t.cancel()


sc = rt.scenegen.room_scene(args.triangles, seed=21, n_lights=4, n_materials=6, tex_size=16, n_tex_sets=2, alpha_fraction=0.2)
dev, _ = step("rt_create", lambda: rt.DeviceScene(sc))
N, K = args.points, args.spp
rng = np.random.default_rng(1)
P = sc.positions.reshape(-1, 3)
o = rng.uniform(P.min(axis=0), P.max(axis=0), size=(N + N // 4, 3)).astype(np.float32)
d = rng.normal(size=o.shape).astype(np.float32)
d /= np.linalg.norm(d, axis=1, keepdims=True)
(prim, bct), _ = step("cast_rays", lambda: dev.cast_rays(np.concatenate([o, d], axis=1)))
hit = np.nonzero(prim != 0xFFFFFFFF)[0][:N]
assert len(hit) == N, f"only {len(hit)} of {N} points"
tri = sc.positions.reshape(-1, 3, 3)[prim[hit]].astype(np.float64)
g = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
g /= np.linalg.norm(g, axis=1, keepdims=True)
g *= -np.sign(np.sum(g * d[hit], axis=1, keepdims=True))
pts = rt.pack_bake_points((o[hit] + bct[hit, 2:3] * d[hit]).astype(np.float32), g.astype(np.float32))
OFFSET, SEED = 1e-3, 1

d_pts = torch.from_numpy(pts.view(np.uint8).copy()).cuda()
d_rays = torch.zeros(N * K * 32, dtype=torch.uint8, device="cuda")
d_out = torch.zeros(N * 27, dtype=torch.float32, device="cuda")
d_per_ray = torch.zeros(N * K * 3, dtype=torch.float32, device="cuda")
torch.cuda.synchronize()

say(f"# tools/bake_bench.py  kernel_src_sha16 {bench.kernel_source_hash()}  library {rt.lib().rt_source_stamp().decode()}  room_scene({args.triangles}), "
    f"{N} points x {K} samples = {N * K / 1e6:.1f} M paths, parity traversal, {args.repeat} interleaved rounds after one warm-up each; ms per call, wall")


def measure(kind):
    sh = kind == "SH9"
    g_out = 1 if sh else K

    def a():
        f = dev.bake_sh if sh else dev.bake_irradiance
        kw = {} if sh else {"offset": OFFSET}
        return f(None, K, seed=SEED, device_points=d_pts.data_ptr(), n_points=N, device_out=d_out.data_ptr(), **kw)[1]

    def b():
        dev.bake_rays(None, K, seed=SEED, sh=sh, offset=OFFSET, device_points=d_pts.data_ptr(), n_points=N, device_out=d_rays.data_ptr())
        return dev.render_rays(None, samples=1, rays_per_output=g_out, seed=SEED, device_rays=d_rays.data_ptr(), n_rays=N * K, device_out=d_per_ray.data_ptr())[1]

    host_rays, _ = step(f"{kind}: rays to the host", lambda: dev.bake_rays(pts, K, seed=SEED, sh=sh, offset=OFFSET))

    def c():
        return dev.render_rays(host_rays, samples=1, rays_per_output=g_out, seed=SEED)[1]

    runs = {"a": [], "b": [], "c": []}
    stats = {}
    for name, fn in (("a", a), ("b", b), ("c", c)):
        step(f"{kind} warm-up {name}", fn)
    for i in range(args.repeat):
        for name, fn in (("a", a), ("b", b), ("c", c)):
            st, ms = step(f"{kind} {name} {i}", fn)
            runs[name].append(ms)
            stats[name] = st
    label = {"a": "rt_bake, device buffers", "b": "rt_bake_rays + rt_render_rays, device buffers", "c": "rt_render_rays, rays from the host"}
    for name in "abc":
        v = runs[name]
        st = stats[name]
        say(f"{kind:10s} {name}  {label[name]:48s} median {statistics.median(v):9.2f}  runs: {' '.join(f'{x:.2f}' for x in v)}   last: kernel_ms {st['kernel_ms']:.2f}, "
            f"wf_extend* {st['dominant_ms']:.2f}, {st['passes']} passes")
    st = stats["a"]
    say(f"{kind:10s} rt_bake: {100 * (st['kernel_ms'] - st['dominant_ms']) / st['kernel_ms']:.2f} % of kernel_ms outside the closest-hit launches "
        f"({st['kernel_ms'] - st['dominant_ms']:.2f} of {st['kernel_ms']:.2f} ms; rt_render_rays over the same rays (b): "
        f"{100 * (stats['b']['kernel_ms'] - stats['b']['dominant_ms']) / stats['b']['kernel_ms']:.2f} %)")
    say(f"{kind:10s} a / b (medians): {statistics.median(runs['a']) / statistics.median(runs['b']):.4f}   a / c: {statistics.median(runs['a']) / statistics.median(runs['c']):.4f}")
    del host_rays


measure("IRRADIANCE")
measure("SH9")

# the rasteriser: every triangle of the scene in its own grid cell of the atlas
T = sc.positions.reshape(-1, 9).astype(np.float32)
n = len(T)
cells = int(np.ceil(np.sqrt(n)))
i = np.arange(n)
corner = np.array([[0.08, 0.08], [0.92, 0.1], [0.1, 0.92]])
uv = np.stack([((i % cells)[:, None] + corner[None, :, 0]) / cells, ((i // cells)[:, None] + corner[None, :, 1]) / cells], axis=2).reshape(n, 6).astype(np.float32)
t3 = T.reshape(n, 3, 3).astype(np.float64)
gn = np.cross(t3[:, 1] - t3[:, 0], t3[:, 2] - t3[:, 0])
gn /= np.maximum(np.linalg.norm(gn, axis=1, keepdims=True), 1e-30)
Nn = np.repeat(gn[:, None, :], 3, axis=1).reshape(n, 9).astype(np.float32)
A = args.atlas
dT, dN, dU = (torch.from_numpy(x).cuda() for x in (T, Nn, uv))
d_lp = torch.zeros(A * A * 8, dtype=torch.int32, device="cuda")
d_lt = torch.zeros(A * A, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
lm = lambda: dev.lightmap_points(dT, dN, dU, A, A, device_points=d_lp.data_ptr(), device_texels=d_lt.data_ptr())
count, _ = step("lightmap warm-up", lm)
v = [step(f"lightmap {k}", lm)[1] for k in range(args.repeat)]
say(f"rt_lightmap_points {A} x {A}, {n} triangles in a {cells} x {cells} grid, device arrays: {count} points, median {statistics.median(v):.3f} ms  runs: {' '.join(f'{x:.3f}' for x in v)}")
dev.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
