"""The motion-vector rule of include/rt_abi.h (rt_accum_attach_flow) as a host model, for exact comparisons with the device (a plain module
next to the tests, like sensor_replay.py and shutter_replay.py).

Points, the pinhole / thin-lens and orthographic projections, the flow of a sample and the per-pixel fold are numpy float32, one operation
per statement: every array is float32 and every scalar operand an np.float32, so each statement rounds once, as the device's does
(-ffp-contract=off). The equirect and fisheye projections need the restated atan2f / asinf of rt_devspec.h, which numpy does not have:
they go through tests/flow_shim.c, the spec header include/rt_flowspec.h itself compiled with the host compiler. The shim evaluates the other
three kinds too, so the CPU tests can hold the numpy statements and the header against each other bit for bit."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import sensor_replay as SR

f32 = np.float32
PI_F = f32(3.14159265358979323846)
PINHOLE, EQUIRECT, FISHEYE, ORTHOGRAPHIC, THIN_LENS = range(5)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, NEAREST = 0, 1


class FlowView(C.Structure):  # rt_flow_view of include/rt_flowspec.h
    _fields_ = [("P", C.c_float * 3), ("R", C.c_float * 3), ("U", C.c_float * 3), ("F", C.c_float * 3), ("tan_x", C.c_float), ("tan_y", C.c_float),
                ("half_fov", C.c_float), ("half_width", C.c_float), ("half_h", C.c_float), ("kind", C.c_uint32)]


def view_of(sensor, W, H):
    """What proj reads of `sensor` (an object with camera / kind / half_width, e.g. the package's Sensor) at a W x H image: the frame as given
    and the hoisted terms of rt::make_sensor, in its float expressions."""
    cam = sensor.camera
    v = {k: np.asarray(getattr(cam, n), dtype=f32).reshape(3) for k, n in (("P", "position"), ("R", "right"), ("U", "up"), ("F", "forward"))}
    v["tan_x"], v["tan_y"] = SR.tangents(cam.fov_x, W, H)
    v["half_fov"] = f32(f32(cam.fov_x) / f32(2))
    hw = f32(getattr(sensor, "half_width", 0.0) or 0.0)
    v["half_width"] = hw
    v["half_h"] = f32(f32(hw * f32(H)) / f32(W))
    v["kind"] = int(sensor.kind)
    return v


def _c_view(v):
    c = FlowView()
    for k in ("P", "R", "U", "F"):
        for i in range(3):
            getattr(c, k)[i] = float(v[k][i])
    c.tan_x, c.tan_y, c.half_fov, c.half_width, c.half_h, c.kind = (float(v["tan_x"]), float(v["tan_y"]), float(v["half_fov"]), float(v["half_width"]),
                                                                  float(v["half_h"]), int(v["kind"]))
    return c


_shim = None


def shim():
    """tests/flow_shim.c over include/rt_flowspec.h, compiled once per process with the host compiler into a temporary directory."""
    global _shim
    if _shim is None:
        out = os.path.join(tempfile.mkdtemp(prefix="flow_shim_"), "libflow_shim.so")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "flow_shim.c"),
                               "-o", out])
        _shim = C.CDLL(out)
    return _shim


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def proj_spec(view, W, H, X):
    """proj of the spec header: (fx, fy, ok) of the points X (n, 3)."""
    X = np.ascontiguousarray(X, dtype=f32).reshape(-1, 3)
    n = X.shape[0]
    fx, fy, ok = np.zeros(n, dtype=f32), np.zeros(n, dtype=f32), np.zeros(n, dtype=np.int32)
    cv = _c_view(view)
    shim().flow_shim_proj(C.byref(cv), C.c_uint32(W), C.c_uint32(H), _fp(X), C.c_uint32(n), _fp(fx), _fp(fy), ok.ctypes.data_as(C.POINTER(C.c_int32)))
    return fx, fy, ok != 0


def _dot(v, a):
    s = v[:, 0] * a[0]
    s = s + v[:, 1] * a[1]
    return s + v[:, 2] * a[2]


def proj(view, W, H, X):
    """proj of the rule: numpy float32 for PINHOLE, THIN_LENS and ORTHOGRAPHIC, the spec header for EQUIRECT and FISHEYE."""
    kind = view["kind"]
    if kind in (EQUIRECT, FISHEYE):
        return proj_spec(view, W, H, X)
    X = np.asarray(X, dtype=f32).reshape(-1, 3)
    v = X - view["P"][None, :]
    r, u, f = _dot(v, view["R"]), _dot(v, view["U"]), _dot(v, view["F"])
    ok = f > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == ORTHOGRAPHIC:
            nx = r / view["half_width"]
            ny = (-u) / view["half_h"]
        else:
            nx = r / f
            nx = nx / view["tan_x"]
            ny = u / f
            ny = (-ny) / view["tan_y"]
        fx = nx + f32(1)
        fx = fx * f32(f32(0.5) * f32(W))
        fy = ny + f32(1)
        fy = fy * f32(f32(0.5) * f32(H))
    assert fx.dtype == f32 and fy.dtype == f32
    return fx, fy, ok


def tri_point(v9, b, c):
    """(V0 * ((1 - b) - c) + V1 * b) + V2 * c per component: v9 (n, 9), b and c (n,) -> (n, 3)"""
    v9 = np.asarray(v9, dtype=f32).reshape(-1, 3, 3)
    a = f32(1) - b
    a = a - c
    x = v9[:, 0, :] * a[:, None]
    x = x + v9[:, 1, :] * b[:, None]
    x = x + v9[:, 2, :] * c[:, None]
    assert x.dtype == f32
    return x


def ray_point(o, d, t):
    x = d * t[:, None]
    return (o + x).astype(f32)


def points(rays, prim, bct, key0, key1, n_triangles):
    """(X0, X1, hit) of the samples whose primary rays are `rays` (RAY_DTYPE records) and whose closest hits are (prim, bct) as rt_cast_rays
    reports them: prim the original triangle index, n_triangles + i for analytic primitive i, 0xFFFFFFFF for a miss. key0 / key1: (n, 9)
    positions, or None where no triangle moves."""
    o, d = np.asarray(rays["origin"], dtype=f32), np.asarray(rays["dir"], dtype=f32)
    b, c, t = (np.ascontiguousarray(bct[:, i], dtype=f32) for i in range(3))
    hit = prim != 0xFFFFFFFF
    X0 = ray_point(o, d, t)
    X1 = X0.copy()
    if key0 is not None:
        tri = hit & (prim < n_triangles)
        idx = np.where(tri, prim, 0).astype(np.int64)
        k0, k1 = np.asarray(key0, dtype=f32).reshape(-1, 9), np.asarray(key1, dtype=f32).reshape(-1, 9)
        X0 = np.where(tri[:, None], tri_point(k0[idx], b, c), X0)
        X1 = np.where(tri[:, None], tri_point(k1[idx], b, c), X1)
    return X0.astype(f32), X1.astype(f32), hit


def sample_flow(view0, view1, W, H, X0, X1, hit):
    """(dx, dy, valid) of the rule for samples with the points X0, X1 (n, 3) and the hit flags `hit`."""
    fx0, fy0, ok0 = proj(view0, W, H, X0)
    fx1, fy1, ok1 = proj(view1, W, H, X1)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = fx1 - fx0
        dy = fy1 - fy0
        if view0["kind"] == EQUIRECT:
            half = f32(f32(0.5) * f32(W))
            dx = np.where(dx > half, dx - f32(W), np.where(dx < -half, dx + f32(W), dx)).astype(f32)
    valid = hit & ok0 & ok1 & np.isfinite(dx) & np.isfinite(dy)
    return dx, dy, valid


def fold(dx, dy, t, valid, state=None):
    """The per-pixel fold over samples in sample order: dx, dy, t, valid are (P, n). Returns the state dict {flow_sum (P, 2), valid (P,),
    near_flow (P, 2), near_t (P,)}; `state`: continue from an earlier one."""
    P, n = dx.shape
    if state is None:
        state = dict(flow_sum=np.zeros((P, 2), dtype=f32), valid=np.zeros(P, dtype=np.uint32), near_flow=np.zeros((P, 2), dtype=f32), near_t=np.zeros(P, dtype=f32))
    FS, m, NF, NT = state["flow_sum"].copy(), state["valid"].copy(), state["near_flow"].copy(), state["near_t"].copy()
    for s in range(n):
        v = valid[:, s]
        with np.errstate(invalid="ignore", over="ignore"):  # an invalid sample's terms are computed and not taken
            FS[:, 0] = np.where(v, FS[:, 0] + dx[:, s], FS[:, 0])
            FS[:, 1] = np.where(v, FS[:, 1] + dy[:, s], FS[:, 1])
        take = v & ((m == 0) | (t[:, s] < NT))
        NF[:, 0] = np.where(take, dx[:, s], NF[:, 0])
        NF[:, 1] = np.where(take, dy[:, s], NF[:, 1])
        NT = np.where(take, t[:, s], NT).astype(f32)
        m = m + v.astype(np.uint32)
    assert FS.dtype == f32 and NF.dtype == f32 and NT.dtype == f32
    return dict(flow_sum=FS, valid=m, near_flow=NF, near_t=NT)


def resolve(state, n, mode):
    """(flow (P, 2), mask (P,)) of a state whose pixels hold n (P,) samples."""
    m = state["valid"]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = state["flow_sum"] / m.astype(f32)[:, None]
        mask = np.where(n != 0, m.astype(f32) / n.astype(f32), f32(0)).astype(f32)
    flow = np.where((m != 0)[:, None], state["near_flow"] if mode == NEAREST else mean, f32(0)).astype(f32)
    return flow, mask
