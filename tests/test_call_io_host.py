"""csrc/rt_call_io.h on the CPU: rt::CallIo (the arrays of one entry-point call, on the host or in the caller's HBM) and rt::queue_and_wait,
run against a stub runtime with a deferred stream under the address and undefined-behaviour sanitizers. Nothing on a GPU machine makes a
copy, a launch or a synchronise fail, so no GPU test runs the paths behind such a failure; here every runtime call of a call fails in turn."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing-course-hw-public_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "call_io_host_main.cpp")  # the stand-alone program: the stub runtime, the scenarios and their checks
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")  # headers only: no HIP runtime is linked


def test_nothing_is_in_flight_on_any_path(tmp_path):
    exe = str(tmp_path / "call_io_host")
    subprocess.check_call(["g++", "-std=c++20", "-g", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", HIP_INCLUDE, "-I", CSRC,
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", MAIN, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stderr  # a failed CHECK, the stub's abort (a free under work in flight, a double free) or a sanitizer report
    assert r.stderr == ""
    lines = r.stdout.splitlines()
    assert re.fullmatch(r"call_io ok: \d+ checks", lines[-1])
    # a host call makes seven runtime calls (allocate, two uploads, the launch, two copies back: none for the null destination, the wait), a
    # device call two; one line for the success and one per failing position. Whatever was queued before a failure is waited for: every
    # sequence that queued something ends in a synchronise, ahead of the free.
    host = [l.rsplit(" ", 1)[1] for l in lines if l.startswith("host call")]
    device = [l.rsplit(" ", 1)[1] for l in lines if l.startswith("device call")]
    assert host == ["MUUKDDSF", "m", "MuSF", "MUuSF", "MUUkSF", "MUUKdSF", "MUUKDdSF", "MUUKDDsF"]  # F: the owner dies after the call
    assert device == ["KS", "kS", "Ks"]
    assert any(l == "growth: calls MUUKDDSFMUUKDDSUUKDDS" for l in lines)
