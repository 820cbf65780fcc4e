"""csrc/rt_wf_policy.h on the CPU: what launch_wavefront_pass decides per bounce (the bound one bounce late, sorted or identity order, keys and
pad fill from the producer, the end of the pass) for every ray depth and every non-increasing sequence of queue sizes around the thresholds,
and the grid helpers against the expressions they replaced; under the address and undefined-behaviour sanitizers. The checks themselves are
tests/wf_policy_host_main.cpp's."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing-course-hw-public_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "wf_policy_host_main.cpp")


def test_every_pass_keeps_the_sort_contract(tmp_path):
    exe = str(tmp_path / "wf_policy_host")
    subprocess.check_call(["g++", "-std=c++20", "-g", "-O1", "-Wall", "-Werror", "-I", CSRC, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", MAIN, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stderr  # a failed CHECK or a sanitizer report
    assert r.stderr == ""
    lines = r.stdout.splitlines()
    assert re.fullmatch(r"wf_policy ok: \d+ checks", lines[-1])
    # every sequence of 1 .. 32 sizes out of ten values, with and without the read-back: 2 * (C(42, 10) - 1)
    assert lines[0] == "policy: 2942885944 passes walked"
