"""The host half of rt_create on the CPU (csrc/rt_scene_prepare.cpp, csrc/rt_tex_views.h), as a stand-alone program under the address and
undefined-behaviour sanitizers: tests/scene_prepare_host_main.cpp.

(a) rt::assign_texture_views against a restatement of its contract, for 1x1, 5x3 and 8x8 textures of random content in fourteen slot
    layouts: every view decodes to its texture, tex_set is set exactly when one record group serves all present slots, regions are disjoint
    and 128-byte aligned, view ids are stable.
(b) rt::prepare on the same cases as whole descriptors over a 12-triangle soup in the three host build kinds, and the first refusal of
    descriptors with two planted faults, against tests/golden/prepared_scene.txt. The fixture is the program's own `--record` output, taken
    from the commit its first line names: built with -DPREPARE_ONLY against that commit's csrc/, with its rt_scene.cpp (which held
    rt::prepare then) in place of rt_scene_prepare.cpp, linked against the HIP runtime with the other unresolved symbols ignored.

The program makes no HIP call and runs without a GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing-course-hw-public_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "scene_prepare_host_main.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "prepared_scene.txt")
SOURCES = [MAIN] + [os.path.join(CSRC, f) for f in ("rt_scene_prepare.cpp", "bvh_build.cpp", "wide_build.cpp", os.path.join("host", "film.cpp"))]  # film.cpp: rt::fail
CASES = ("four_slots_one_size", "two_sizes_tie", "all_1x1", "one_texture", "set_starts_at_slot_1", "set_plus_other_size", "same_tuple_twice", "shared_texture_two_tuples",
         "bg_shared_with_material", "bg_alone", "force_tiled", "footprint_cap_0", "budget_below_first_set", "nothing")


def test_view_assignment_and_prepared_scene(tmp_path):
    exe = str(tmp_path / "scene_prepare_host")
    subprocess.check_call(["g++", "-std=c++20", "-g", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", "/opt/rocm/include",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *SOURCES, "-o", exe])
    r = subprocess.run([exe, "--check", GOLDEN], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stderr  # a failed CHECK, a record that differs or a sanitizer report
    assert r.stderr == ""
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith("views ")] == [f"views {c} ok" for c in CASES]
    assert re.fullmatch(r"prepared_scene ok: \d+ records, \d+ checks", lines[-1])
    with open(GOLDEN) as f:
        golden = f.read().splitlines()
    assert re.match(r"# recorded at commit [0-9a-f]{7,40}\b", golden[0])
    assert int(lines[-1].split()[2]) == len(golden) - 1
    assert [l.split()[1:] for l in golden if l.startswith("case ")] == [[c, k] for c in CASES for k in ("flat", "wide", "device")]
    assert sum(l.startswith("refusal ") for l in golden) == 28  # every pair of the seven faults, and each alone
