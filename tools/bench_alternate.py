#!/usr/bin/env python3
"""tools/bench_alternate.py PARENT_TREE — the no-regression record of a pull request: the bench.py headline of a built checkout of the parent
commit against this checkout, alternating (parent, this, parent, this, ...) as child processes of one call, so that both see the same
machine in the same minutes. Appends to profiles/render_rays.txt (--out): every run's value, both medians, their ratio, and the spread of the
repeated parent runs ((max - min) / median), which is the margin the ratio is read against.
Every bench.py runs under --run-timeout in a process group of its own; the first one that does not end with status 0 ends this tool with
that status (124 for a time limit) and nothing more is started."""
import argparse, json, os, signal, statistics, subprocess, sys

ap = argparse.ArgumentParser()
ap.add_argument("parent", help="a built checkout of the parent commit")
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--run-timeout", type=float, default=200.0)
ap.add_argument("--out", default=None, help="default: profiles/render_rays.txt of this checkout")
args = ap.parse_args()

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out_path = args.out or os.path.join(HERE, "profiles", "render_rays.txt")


def headline(tree):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup)]
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=tree, start_new_session=True)
    try:
        out, err = child.communicate(timeout=args.run_timeout)
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        child.wait()
        sys.stderr.write(f"bench_alternate: bench.py in {tree} did not finish within {args.run_timeout:.0f} s; nothing more is started\n")
        sys.exit(124)
    if child.returncode != 0:
        sys.stderr.write(f"bench_alternate: bench.py in {tree} ended with status {child.returncode}; nothing more is started\n{err[-2000:]}\n")
        sys.exit(child.returncode if child.returncode > 0 else 128 - child.returncode)
    j = json.loads(out.strip().splitlines()[-1])
    return float(j["value"]), j


parent, this, meta = [], [], {}
for r in range(args.rounds):
    v, meta["parent"] = headline(os.path.abspath(args.parent))
    parent.append(v)
    print(f"parent {r}: {v:.3f}", flush=True)
    v, meta["this"] = headline(HERE)
    this.append(v)
    print(f"this   {r}: {v:.3f}", flush=True)
mp, mt = statistics.median(parent), statistics.median(this)
spread = (max(parent) - min(parent)) / mp
lines = [
    f"# tools/bench_alternate.py  bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup}, {args.rounds} rounds of (parent, this) in one call; "
    f"metric: {meta['this'].get('metric', '?')} [{meta['this'].get('unit', '?')}]",
    f"parent commit    median {mp:9.3f}  runs: {' '.join(f'{x:.3f}' for x in parent)}",
    f"this commit      median {mt:9.3f}  runs: {' '.join(f'{x:.3f}' for x in this)}",
    f"this / parent (medians): {mt / mp:.4f}   spread of the parent runs (max - min) / median: {spread:.4f} = the margin",
    f"verdict: {'no regression beyond the margin' if mt / mp >= 1 - spread else 'SLOWER than the parent by more than the margin'}",
]
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n")
