"""GPU test of the wavefront pass kinds (csrc/rt_kernels.h WfPassKind): no state leaks from one kind of pass to the next.

Every entry point of the wavefront pipeline describes its passes with one record (cameras, an accumulator's list, a caller's rays, bake points)
and all of them share the scene's workspace, its sensor table, its staging buffers and its camera-relative records. The other GPU files pin
each entry point on its own; here the kinds are interleaved on ONE scene, and every call must give, byte for byte and pass for pass, what it
gives on a scene that ran nothing else. 48 x 32 pixels x 8 samples with max_paths = 1024 (the floor the library accepts): 2 pixel tiles x 8
sample passes for the image entry points, 3 passes for a bake of 300 points, 12 for an accumulator round. All comparisons are on raw bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP = 48, 32, 8
MAX_PATHS = 1024
N_PTS = 300
SEED = 5
BUILDS = {"parity": {}, "production": dict(device_bvh=True, wide=True)}
ORDER = ("bake", "accum", "rays", "sensors", "render", "accum", "bake_sh", "render")  # the second accum is a new accumulator


@pytest.fixture(scope="module")
def scene(sg):
    return sg.room_scene(800, seed=21)


@pytest.fixture(scope="module")
def points(gpu, scene):
    """300 bake points on the scene's own triangles: the centroids of the first 300, with their geometric normals"""
    tri = scene.positions.reshape(-1, 3, 3)[:N_PTS].astype(np.float64)
    assert len(tri) == N_PTS
    g = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    pts = gpu.pack_bake_points(tri.mean(axis=1).astype(np.float32), g.astype(np.float32))
    pts.setflags(write=False)
    return pts


def run_call(gpu, dev, scene, points, name, tuning):
    """One call of the kind `name` on `dev`: its outputs by name (arrays) and the passes it ran"""
    cam = scene.camera
    if name == "render":
        fb, st = dev.run_raytracer(W, H, SPP, seed=SEED, **tuning)
        out = dict(image=fb)
    elif name == "sensors":
        img, st = dev.render_sensors(W, H, SPP, [gpu.Sensor.pinhole(cam, SEED), gpu.Sensor.fisheye(cam, SEED + 1)], **tuning)
        out = dict(images=img)
    elif name == "rays":
        rays = dev.sensor_rays(gpu.Sensor.pinhole(cam, SEED), W, H, samples=SPP)
        rgb, st = dev.render_rays(rays, samples=1, rays_per_output=SPP, seed=SEED, **tuning)
        out = dict(rays=rays, outputs=rgb)
    elif name == "bake":
        e, st = dev.bake_irradiance(points, SPP, seed=SEED, offset=1e-3, **tuning)
        out = dict(irradiance=e)
    elif name == "bake_sh":
        sh, st = dev.bake_sh(points, SPP, seed=SEED, **tuning)
        out = dict(sh=sh)
    else:
        assert name == "accum"
        acc = dev.accumulator(W, H, seed=SEED, features=True, ids="primitive")
        st = acc.render(SPP, **tuning)
        out = dict(image=acc.image(), **acc.read_features(), **acc.read_ids())
        acc.close()
    return {k: np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy() for k, v in out.items()}, st["passes"]  # raw bytes, one row


@pytest.fixture(scope="module", params=list(BUILDS))
def build(request):
    return request.param


@pytest.fixture(scope="module", params=["packet_auto", "packet_on"])
def tuning(request, gpu):
    t = dict(max_paths=MAX_PATHS)
    if request.param == "packet_on":  # camera-relative records between kinds that may not use them
        t["packet_mode"] = gpu.RT_PACKET_ON
    return t


@pytest.fixture(scope="module")
def references(gpu, scene, points, build, tuning):
    """kind -> (outputs, passes) of the call on a scene of its own; computed once, never written to"""
    refs = {}
    for name in sorted(set(ORDER)):
        dev = gpu.DeviceScene(scene, **BUILDS[build])
        refs[name] = run_call(gpu, dev, scene, points, name, tuning)
        dev.close()
        for a in refs[name][0].values():
            a.setflags(write=False)
    return refs


def test_references_have_the_planned_passes(references):
    """the shape does what the docstring says: every kind runs several passes, so the pass loop and the workspace rebinding are exercised"""
    assert {k: v[1] for k, v in references.items()} == dict(render=16, sensors=24, rays=16, bake=3, bake_sh=3, accum=12)


def test_rays_of_the_camera_give_the_render(references):
    assert np.array_equal(references["rays"][0]["outputs"], references["render"][0]["image"])


def test_interleaved_kinds_equal_their_references(gpu, scene, points, build, tuning, references):
    dev = gpu.DeviceScene(scene, **BUILDS[build])
    try:
        got = {}
        for step, name in enumerate(ORDER):
            out, passes = run_call(gpu, dev, scene, points, name, tuning)
            ref, ref_passes = references[name]
            assert passes == ref_passes, (step, name)
            assert out.keys() == ref.keys()
            for k in ref:
                assert np.array_equal(out[k], ref[k]), (step, name, k, int(np.count_nonzero(out[k] != ref[k])))
            got[name] = out
        # the documented identity, across interleaved kinds: a camera's own rays give its image
        assert np.array_equal(got["rays"]["outputs"], got["render"]["image"])
    finally:
        dev.close()
