#!/usr/bin/env python3
"""tools/render_rays_bench.py — what rt_render_rays costs beside rt_render (DESIGN.md "Caller-supplied rays"): writes profiles/render_rays.txt.

On the sponza-like scene of bench.make_scene at --size x --size x --spp (512 x 512 x 16), with rays.pinhole rays of the scene's camera in a
device buffer and device outputs, one process:
  * rt_render_rays (samples = 1, rays_per_output = spp) and rt_render of the same shape take turns, --repeat times after one warm-up each;
    Msamples/s of both from the device time of each call (rt_stats.kernel_ms), best and median;
  * the share of the rays first stage (wf_first_stage<., ., WfFromRays>) in the device time of rt_render_rays' kernels: a child process (this file with --child) that only renders
    rays, under `rocprofv3 --kernel-trace --stats`, started BEFORE this process touches the GPU, in a process group of its own; if it does
    not end with status 0 this process ends with its status (124 for a time limit) and starts nothing on the GPU.
Every GPU step of this process runs under --step-timeout too (a watchdog ends the process: a hung step must not be waited for).
--tree DIR imports bench.py and the package from another built checkout (a parent commit has no rt_render_rays: only rt_render is timed)."""
import argparse, csv, glob, importlib, os, shutil, signal, statistics, subprocess, sys, tempfile, threading

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--spp", type=int, default=16)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a single GPU step (rt_create, one render) may take; the profiled child gets this for each of its steps")
ap.add_argument("--tree", default=None, help="another built checkout to time rt_render on")
ap.add_argument("--out", default=None, help="default: profiles/render_rays.txt of this checkout")
ap.add_argument("--append", action="store_true")
ap.add_argument("--no-kernel-share", action="store_true")
ap.add_argument("--rays-packet-mode", type=int, default=0, help="rt_params.packet_mode of the rt_render_rays calls (RT_PACKET_*: 0 auto, 1 off, 2 on)")
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(args.tree) if args.tree else HERE
out_path = args.out or os.path.join(HERE, "profiles", "render_rays.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


CHILD_REPEAT = 2


def kernel_share():
    """(share, total ms, per-kernel rows) of the child's kernels. The child has the GPU open: if it does not end with status 0 (a fault, an
    abort, a time limit) this process ends with the child's status, or 124, and starts nothing on the GPU. The child runs in a process group
    of its own, so that a time limit ends the profiler AND the program under it."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 not found", []
    d = tempfile.mkdtemp(prefix="render_rays_prof_")
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", "--size", str(args.size),
           "--spp", str(args.spp), "--repeat", str(CHILD_REPEAT), "--step-timeout", str(args.step_timeout)]
    limit = args.step_timeout * (3 + CHILD_REPEAT)  # scene set-up, rt_create, 1 + CHILD_REPEAT renders: each has its own limit inside the child
    try:
        child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=d, start_new_session=True)
        try:
            log, _ = child.communicate(timeout=limit)
        except subprocess.TimeoutExpired:
            os.killpg(child.pid, signal.SIGKILL)
            child.wait()
            sys.stderr.write(f"render_rays_bench: the profiled child did not finish within {limit:.0f} s; nothing more is started on the GPU\n")
            sys.exit(124)
        if child.returncode != 0:
            sys.stderr.write(f"render_rays_bench: the profiled child ended with status {child.returncode}; nothing more is started on the GPU\n" + log[-2000:] + "\n")
            sys.exit(child.returncode if child.returncode > 0 else 128 - child.returncode)
        files = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)
        if not files:
            return None, "the profiler wrote no kernel_stats.csv", []
        rows = list(csv.DictReader(open(files[0])))
        total = sum(float(x["TotalDurationNs"]) for x in rows)
        gen = sum(float(x["TotalDurationNs"]) for x in rows if "wf_first_stage" in x["Name"] and "WfFromRays" in x["Name"])
        return gen / total, total / 1e6, sorted(rows, key=lambda x: -float(x["TotalDurationNs"]))[:6]
    finally:
        shutil.rmtree(d, ignore_errors=True)


share = None
if not args.child and not args.tree and not args.no_kernel_share:
    share = kernel_share()  # before this process opens the GPU

sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (before the library: bench.py's rule)
import bench

rt = importlib.import_module("raytracing-course-hw-public_amd")


def step(what, fn):
    """One GPU step under its own time limit: a step that outlives it ends the process (status 124), nothing is retried."""
    def expired():
        sys.stderr.write(f"render_rays_bench: step '{what}' exceeded {args.step_timeout:.0f} s\n")
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
sc = bench.make_scene(rt, wl, wl["triangles"], wl["tex_size"], W / H)
dev = step("rt_create", lambda: rt.DeviceScene(sc))
has_rays = hasattr(rt.DeviceScene, "render_rays")
n_out, n = W * H, W * H * args.spp
d_fb = torch.zeros(n_out * 3, dtype=torch.float32, device="cuda")
if has_rays:
    packed = rt.rays.pinhole(sc.camera, W, H, args.spp, seed=1)
    d_rays = torch.from_numpy(np.frombuffer(packed.tobytes(), dtype=np.uint8).copy()).cuda()
    d_out = torch.zeros(n_out * 3, dtype=torch.float32, device="cuda")
torch.cuda.synchronize()


def rays_once():
    return dev.render_rays(None, samples=1, rays_per_output=args.spp, seed=1, device_rays=d_rays.data_ptr(), device_out=d_out.data_ptr(), n_rays=n, packet_mode=args.rays_packet_mode)[1]


def render_once():
    return dev.run_raytracer(W, H, args.spp, seed=1, device_fb=d_fb.data_ptr())[1]


if args.child:  # under the profiler: only rt_render_rays
    for i in range(1 + args.repeat):
        step(f"rt_render_rays {i}", rays_once)
    dev.close()
    sys.exit(0)

say(f"# tools/render_rays_bench.py  tree {'parent checkout' if args.tree else 'this checkout'}  kernel_src_sha16 {bench.kernel_source_hash()}  library {rt.lib().rt_source_stamp().decode()}"
    f"  {wl['label']} {W}x{H}x{args.spp}, parity traversal, device buffers, rt_render_rays packet_mode {args.rays_packet_mode}, {args.repeat} alternating runs after one warm-up each")
if has_rays:
    step("warm-up rt_render_rays", rays_once)
step("warm-up rt_render", render_once)
t_rays, t_render, last = [], [], {}
for i in range(args.repeat):
    if has_rays:
        st = step(f"rt_render_rays {i}", rays_once)
        t_rays.append(st["samples"] / st["kernel_ms"] / 1e3)
        last["rt_render_rays"] = st
    st = step(f"rt_render {i}", render_once)
    t_render.append(st["samples"] / st["kernel_ms"] / 1e3)
    last["rt_render"] = st


def line(name, v):
    say(f"{name:16s} best {max(v):8.1f}  median {statistics.median(v):8.1f}  worst {min(v):8.1f} Msamples/s   runs: {' '.join(f'{x:.1f}' for x in v)}")
    st = last[name]  # which closest-hit kernel the primary rays of the last run took: the two entry points keep separate packet policies
    say(f"{'':16s} last run: {st['packet_passes']} of {st['passes']} passes through the packet kernel, {st['packet_lanes_x100'] / 100:.1f} lanes per packet trip, wf_extend* {st['dominant_ms']:.2f} of {st['kernel_ms']:.2f} ms")


if has_rays:
    line("rt_render_rays", t_rays)
line("rt_render", t_render)
if has_rays:
    say(f"rt_render_rays / rt_render (medians): {statistics.median(t_rays) / statistics.median(t_render):.4f}   "
        f"(the same camera model with numpy's jitter instead of gen_ray's: nearly, not exactly, the same paths)")
if share is not None:
    if share[0] is None:
        say(f"rays first stage share: not measured ({share[1]})")
    else:
        say(f"rays first stage (wf_first_stage over WfFromRays): {100 * share[0]:.2f} % of the {share[1]:.2f} ms of kernel time of a process that only ran rt_render_rays (rocprofv3 --kernel-trace --stats, {1 + CHILD_REPEAT} calls)")
        for x in share[2]:
            nm = x["Name"]
            nm = nm[nm.find("wf_"):][:44] if "wf_" in nm else nm[:44]
            say(f"    {nm:46s} calls {int(x['Calls']):5d}  total {float(x['TotalDurationNs']) / 1e6:9.2f} ms")
dev.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "a" if args.tree or args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
