"""CPU tests of what rt_bake adds on the host side: the layouts of rt_bake_point and rt_bake_desc as a C compiler sees include/rt_abi.h
against their ctypes and numpy mirrors, the three new symbols, and pack_bake_points."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def abi():
    return importlib.import_module("raytracing-course-hw-public_amd._ctypes_abi")


def test_bake_layouts_match_the_c_header(abi, tmp_path):
    src = tmp_path / "bake.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "rt_abi.h"\nint main(){printf("%zu %zu %zu %zu %zu  %zu %zu %zu %zu %zu  %d %d\\n",'
        "sizeof(rt_bake_point),offsetof(rt_bake_point,position),offsetof(rt_bake_point,normal),offsetof(rt_bake_point,stream),offsetof(rt_bake_point,reserved),"
        "sizeof(rt_bake_desc),offsetof(rt_bake_desc,kind),offsetof(rt_bake_desc,first_sample),offsetof(rt_bake_desc,offset),offsetof(rt_bake_desc,reserved),"
        "(int)RT_BAKE_IRRADIANCE,(int)RT_BAKE_SH9);return 0;}\n"
    )
    exe = tmp_path / "bake"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])  # C, not C++: the header is a C header
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [32, 0, 12, 24, 28, 32, 0, 4, 8, 12, 0, 1]
    P = abi.RtBakePoint
    assert got[:5] == [ctypes.sizeof(P), P.position.offset, P.normal.offset, P.stream.offset, P.reserved.offset]
    D = abi.BAKE_POINT_DTYPE
    assert got[:5] == [D.itemsize] + [D.fields[k][1] for k in ("position", "normal", "stream", "reserved")]
    B = abi.RtBake
    assert got[5:10] == [ctypes.sizeof(B), B.kind.offset, B.first_sample.offset, B.offset.offset, B.reserved.offset]
    assert got[10:] == [abi.RT_BAKE_IRRADIANCE, abi.RT_BAKE_SH9]


def test_the_library_exports_the_bake_entry_points(rt, abi):
    lib = rt.lib()
    for name in ("rt_bake", "rt_bake_rays", "rt_lightmap_points"):
        assert name in abi.ABI_PROTOTYPES and getattr(lib, name) is not None
    assert lib.rt_abi_version() == 4  # additive


def test_pack_bake_points_defaults_and_packed_forms(rt, abi):
    pos = np.arange(15, dtype=np.float64).reshape(5, 3)
    p = rt.pack_bake_points(pos)
    assert p.dtype == abi.BAKE_POINT_DTYPE and p.flags["C_CONTIGUOUS"] and len(p) == 5
    assert np.array_equal(p["position"], pos.astype(np.float32)) and np.all(p["normal"] == 0) and np.all(p["reserved"] == 0)
    assert np.array_equal(p["stream"], np.arange(5))  # the default stream is the index
    nrm = np.tile([0.0, 1.0, 0.0], (5, 1))
    q = rt.pack_bake_points(pos, nrm, stream=[9, 8, 7, 6, 2 ** 32 - 1])
    assert np.array_equal(q["normal"], nrm.astype(np.float32)) and list(q["stream"]) == [9, 8, 7, 6, 2 ** 32 - 1]
    assert np.array_equal(rt.pack_bake_points(q).view(np.uint32), q.view(np.uint32))  # packed records pass through
    assert rt.pack_bake_points(q[::2]).flags["C_CONTIGUOUS"]
    c = (abi.RtBakePoint * 2)()
    c[1].position[2], c[1].normal[0], c[1].stream = 3.0, -1.0, 77
    v = rt.pack_bake_points(c)
    assert len(v) == 2 and v["position"][1, 2] == 3.0 and v["normal"][1, 0] == -1.0 and v["stream"][1] == 77
    with pytest.raises(ValueError):
        rt.pack_bake_points(q, stream=np.zeros(5))
    assert len(rt.pack_bake_points(np.zeros((0, 3)))) == 0
