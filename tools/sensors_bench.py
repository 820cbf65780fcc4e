#!/usr/bin/env python3
"""tools/sensors_bench.py — what the device-side sensor models cost (DESIGN.md "Sensor models"): appends to profiles/sensors.txt.

On the sponza-like scene of bench.make_scene at --size x --size x --spp (512 x 512 x 16), device output buffers, one process, Msamples/s
from the device time of each call (rt_stats.kernel_ms), --repeat alternating runs after one warm-up each, best / median / worst:
  (b) rt_render_sensors with one PINHOLE sensor against rt_render_views with that camera and seed: the same kernels behind a first stage
      that reads a 128-byte record instead of a 64-byte one;
  (c) every other kind against rt_render_rays (samples = 1, rays_per_output = spp) over that sensor's own rays, written once into a device
      buffer by rt_sensor_rays: the same paths, so the difference is the first stage alone (a 32-byte read per path saved, the sensor's
      arithmetic paid).
(a), the bench.py headline of the parent commit against this one, is tools/bench_alternate.py PARENT --out profiles/sensors.txt.
Every GPU step runs under --step-timeout: a step that outlives it ends the process (status 124); nothing is retried."""
import argparse, importlib, os, statistics, sys, threading

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--step-timeout", type=float, default=120.0)
ap.add_argument("--out", default=None, help="default: profiles/sensors.txt of this checkout")
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = args.out or os.path.join(HERE, "profiles", "sensors.txt")
sys.path.insert(0, HERE)
import torch  # noqa: E402  (before the library: bench.py's rule)
import bench  # noqa: E402

rt = importlib.import_module("raytracing-course-hw-public_amd")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def step(what, fn):
    def expired():
        sys.stderr.write(f"sensors_bench: step '{what}' exceeded {args.step_timeout:.0f} s\n")
        sys.stderr.flush()
        os._exit(124)

    t = threading.Timer(args.step_timeout, expired)
    t.daemon = True
    t.start()
    try:
        return fn()
    finally:
        t.cancel()


wl = bench.WORKLOADS["sponza"]
W = H = args.size
SPP, SEED = args.spp, 1
sc = bench.make_scene(rt, wl, wl["triangles"], wl["tex_size"], W / H)
dev = step("rt_create", lambda: rt.DeviceScene(sc))
n_out, n = W * H, W * H * SPP
d_a = torch.zeros(n_out * 3, dtype=torch.float32, device="cuda")
d_b = torch.zeros(n_out * 3, dtype=torch.float32, device="cuda")
d_rays = torch.zeros(n * 8, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
cam = sc.camera
extent = float(abs(sc.positions.reshape(-1, 3)).max())
sensors = {
    "pinhole": rt.Sensor.pinhole(cam, seed=SEED),
    "equirect": rt.Sensor.equirect(cam, seed=SEED),
    "fisheye": rt.Sensor.fisheye(cam, seed=SEED),
    "orthographic": rt.Sensor.orthographic(cam, half_width=0.25 * extent, seed=SEED),
    "thin_lens": rt.Sensor.thin_lens(cam, lens_radius=0.01 * extent, focus_distance=0.5 * extent, seed=SEED),
}


def rate(st):
    return st["samples"] / st["kernel_ms"] / 1e3


def alternate(name_a, fn_a, name_b, fn_b):
    step(f"warm-up {name_a}", fn_a)
    step(f"warm-up {name_b}", fn_b)
    ra, rb, last = [], [], {}
    for i in range(args.repeat):
        last[name_a] = step(f"{name_a} {i}", fn_a)
        ra.append(rate(last[name_a]))
        last[name_b] = step(f"{name_b} {i}", fn_b)
        rb.append(rate(last[name_b]))
    for nm, v in ((name_a, ra), (name_b, rb)):
        st = last[nm]
        say(f"  {nm:34s} best {max(v):8.1f}  median {statistics.median(v):8.1f}  worst {min(v):8.1f} Msamples/s   runs: {' '.join(f'{x:.1f}' for x in v)}"
            f"   [{st['packet_passes']} of {st['passes']} passes as packets, {st['packet_lanes_x100'] / 100:.1f} lanes per trip]")
    say(f"  {name_a} / {name_b} (medians): {statistics.median(ra) / statistics.median(rb):.4f}")
    return ra, rb


say(f"# tools/sensors_bench.py  kernel_src_sha16 {bench.kernel_source_hash()}  library {rt.lib().rt_source_stamp().decode()}  {wl['label']} {W}x{H}x{SPP}, "
    f"parity traversal, device buffers, {args.repeat} alternating runs after one warm-up each")
say("(b) one PINHOLE sensor against rt_render_views of the same camera and seed")
alternate("rt_render_sensors pinhole", lambda: dev.render_sensors(W, H, SPP, [sensors["pinhole"]], device_out=d_a.data_ptr())[1],
          "rt_render_views", lambda: dev.run_raytracer_views(W, H, SPP, [cam], [SEED], device_fb=d_b.data_ptr())[1])
assert torch.equal(d_a.view(torch.int32), d_b.view(torch.int32)), "pinhole sensor != rt_render_views"
say("(c) every other kind against rt_render_rays over the rays rt_sensor_rays wrote for it (the same paths)")
for kind in ("equirect", "fisheye", "orthographic", "thin_lens"):
    sn = sensors[kind]
    step(f"rt_sensor_rays {kind}", lambda: dev.sensor_rays(sn, W, H, SPP, device_out=d_rays.data_ptr()))
    alternate(f"rt_render_sensors {kind}", lambda: dev.render_sensors(W, H, SPP, [sn], device_out=d_a.data_ptr())[1],
              f"rt_render_rays ({kind} rays)", lambda: dev.render_rays(None, samples=1, rays_per_output=SPP, seed=SEED, device_rays=d_rays.data_ptr(),
                                                                        device_out=d_b.data_ptr(), n_rays=n)[1])
    assert torch.equal(d_a.view(torch.int32), d_b.view(torch.int32)), f"{kind}: sensor image != rt_render_rays over its rays"
dev.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n")
