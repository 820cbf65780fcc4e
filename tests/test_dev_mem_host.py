"""csrc/rt_dev_mem.h and csrc/rt_build_host.h on the CPU: the owners of device memory (rt::DevArena, rt::DevBuf, the builders' rt::ScratchArena
that drains its stream before it frees), the two try macros and the builders' read-back and scan total, run against a stub allocator and a stub
stream under the address and undefined-behaviour sanitizers. The failure paths they replace (a free on every return path of every builder) are run
by no GPU test, since nothing there makes an allocation fail; here every allocation of a sequence fails in turn."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracing-course-hw-public_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "dev_mem_host_main.cpp")  # the stand-alone program: the stub runtime, the scenarios and their checks
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")  # headers only: no HIP runtime is linked


def test_owners_free_everything_on_every_path(tmp_path):
    exe = str(tmp_path / "dev_mem_host")
    subprocess.check_call(["g++", "-std=c++20", "-g", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", HIP_INCLUDE, "-I", CSRC,
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", MAIN, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stderr  # a failed CHECK, the stub's abort (double free, unknown pointer) or a sanitizer report
    assert r.stderr == ""
    lines = r.stdout.splitlines()
    assert re.fullmatch(r"dev_mem ok: \d+ checks", lines[-1])
    # one line per failing position of the six-allocation sequence, and one for none: the allocations before the failure, the failure, one
    # free for each of them
    seq = [l for l in lines if l.startswith("arena sequence")]
    assert len(seq) == 7
    for k, l in enumerate(seq):
        calls = l.rsplit(" ", 1)[1]
        assert calls == ("M" * k + "x" + "F" * k if k < 6 else "M" * 6 + "F" * 6), l
    # the builders' steps on a stream (rt_build_host.h), every stubbed call failing in turn: whatever was put on the stream ('C' a copy, 'L' a
    # launch; lower case: the one that failed), one synchronise ('S') follows the last of it and comes directly before the frees
    ok = "MMCLCCSMLCS"
    seq = [l.rsplit(" ", 1)[1] for l in lines if l.startswith("stream sequence")]
    assert len(seq) == len(ok) + 1
    for k, calls in enumerate(seq):
        n_allocs = sum(c == "M" for c in ok[:k])
        head = ok[:k] + ({"M": "x"}.get(ok[k], ok[k].lower()) if k < len(ok) else "")
        assert calls == head + "S" + "F" * n_allocs, (k, calls)


def test_only_the_header_allocates_device_memory():
    """The owners are the only callers of the allocator: a new call site elsewhere would bring back a hand-written free path."""
    offenders = []
    for dirpath, _, names in os.walk(CSRC):
        for n in names:
            if n.endswith((".cpp", ".hip", ".h")) and n != "rt_dev_mem.h":
                text = open(os.path.join(dirpath, n), encoding="utf-8", errors="replace").read()
                if re.search(r"\bhip(Malloc|Free)\(", text):
                    offenders.append(n)
    assert offenders == []


def test_no_entry_point_stages_its_arrays_by_hand():
    """Host or device arrays are one decision, made by rt::CallIo (rt_call_io.h): no entry point picks a pointer or a copy kind by the
    RT_FLAG_DEVICE_FB flag itself, and the per-purpose staging buffers it replaced stay gone. rt_group.cpp keeps its own handling of the
    flag (the RCCL gather)."""
    allowed = {  # file -> the one line that may stay, and why
        "rt_accum_layers.cpp": "device_table ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice",  # attach_arrays: a layer's one table, uploaded into the accumulator's own arena
    }
    gone = re.compile(r"\bensure_fb\b|\bensure_rays\b|s->rgb8\b|s->fb\b")
    pick = re.compile(r"\?\s*hipMemcpy\w+\s*:\s*hipMemcpy\w+|\bdevice_(fb|out)\s*\?")
    offenders = []
    for dirpath, _, names in os.walk(CSRC):
        for n in names:
            if not n.endswith((".cpp", ".hip", ".h")):
                continue
            for no, line in enumerate(open(os.path.join(dirpath, n), encoding="utf-8", errors="replace"), 1):
                if gone.search(line):
                    offenders.append((n, no, "a staging buffer of its own"))
                if n not in ("rt_call_io.h", "rt_group.cpp") and pick.search(line.replace(allowed.get(n, "\0"), "")):
                    offenders.append((n, no, "picks by the flag"))
    assert offenders == []
