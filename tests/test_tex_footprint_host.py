"""csrc/rt_tex_views.h on the CPU: the one builder of the texel pool's layouts (tiled texels, interleaved sets, footprint sets), as a
stand-alone program under the address and undefined-behaviour sanitizers. For 1x1, 1x5, 2x2, 3x7, 4x2, 5x3, 9x8 and 16x16 texels every
base texel's footprint record equals the four records that a plain restatement of TexFoot's neighbour rule reads from the tiled layout, the
pool region is exactly covered, and views over the cap (or of a forced-tiled build) fall back to tiles."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing-course-hw-public_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "tex_footprint_host_main.cpp")  # the stand-alone program: the restatement and its checks


def test_footprint_records_match_the_tiled_neighbours(tmp_path):
    exe = str(tmp_path / "tex_footprint_host")
    subprocess.check_call(["g++", "-std=c++20", "-g", "-O1", "-Wall", "-Werror", "-I", CSRC, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", MAIN, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stderr  # a failed CHECK or a sanitizer report
    assert r.stderr == ""
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith("size ")] == [f"size {s} ok" for s in ("1x1", "1x5", "2x2", "3x7", "4x2", "5x3", "9x8", "16x16")]
    assert re.fullmatch(r"tex_footprint ok: \d+ checks", lines[-1])
