#!/usr/bin/env python3
"""tools/multiview_timing.py — K camera views of one scene in ONE rt_render_views call against K sequential rt_render calls:
the S-sponza scene of bench.make_scene in parity and production builds, K in {1, 2, 4, 8, 16} distinct cameras, at 256 x 256 x 4 and
64 x 64 x 8, with RT_SORT_AUTO (sorts a pass from 2^20 paths up) and RT_SORT_OFF. Best of 20 after 3 warm-up renders, wall and device ms
(rt_stats.kernel_ms, summed over the sequential calls). Also rt_render against a one-view rt_render_views of the same camera."""
import importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import torch  # noqa: F401
import bench
rt = importlib.import_module("raytracing-course-hw-public_amd")
wl = bench.WORKLOADS["sponza"]
sc = bench.make_scene(rt, wl, wl["triangles"], 256, 1.0)
print(f"kernel_src_sha16 {bench.kernel_source_hash()}  library {rt.lib().rt_source_stamp().decode()}")


def cameras(k):
    p = sc.camera.position
    return [rt.scenegen.look_camera(p, yaw_deg=-90.0 + 360.0 * i / 16, yfov=0.9) for i in range(k)]


def best(fn):
    for _ in range(3):
        fn()
    wall, dev = [], []
    for _ in range(20):
        t0 = time.perf_counter(); d = fn(); wall.append(time.perf_counter() - t0); dev.append(d)
    return min(wall) * 1e3, min(dev)


for name, kw in (("parity", {}), ("production", dict(device_bvh=True, wide=True))):
    dev = rt.DeviceScene(sc, **kw)
    for W, H, spp in ((256, 256, 4), (64, 64, 8)):
        one_cam = [sc.camera]
        w1, d1 = best(lambda: dev.run_raytracer(W, H, spp, seed=3)[1]["kernel_ms"])
        w2, d2 = best(lambda: dev.run_raytracer_views(W, H, spp, one_cam, [3])[1]["kernel_ms"])
        print(f"S-sponza {name:10s} {W}x{H}x{spp}: rt_render wall {w1:6.2f} ms device {d1:6.2f} ms | rt_render_views K=1 wall {w2:6.2f} ms device {d2:6.2f} ms")
        for sort_label, sort in (("auto", rt.RT_SORT_AUTO), ("off", rt.RT_SORT_OFF)):
            for k in (1, 2, 4, 8, 16):
                cams, seeds = cameras(k), list(range(k))

                def batch():
                    return dev.run_raytracer_views(W, H, spp, cams, seeds, sort_mode=sort)[1]["kernel_ms"]

                def sequential():
                    return sum(dev.run_raytracer(W, H, spp, seed=s, sort_mode=sort)[1]["kernel_ms"] for s in seeds)

                wb, db = best(batch)
                ws, ds = best(sequential)
                paths = k * W * H * spp
                print(f"S-sponza {name:10s} {W}x{H}x{spp} sort {sort_label:4s} K={k:2d} ({paths:8d} paths): batch wall {wb:7.2f} ms device {db:7.2f} ms | "
                      f"{k:2d} x rt_render wall {ws:7.2f} ms device {ds:7.2f} ms | wall speed-up {ws / wb:5.2f}x")
    dev.close()
