#!/usr/bin/env python3
"""A/B of a change that leaves every kernel's ISA alone (tools/compare_isa.py) and touches host dispatch only: the in-tree library
against one built from the parent commit, through bench.py's render and training-step workloads.  One bench.py process per library,
workload and round (DFN_LIB selects the library).  Each round runs parent, this, parent: the parent's library is measured against
ITSELF in the same session, and its run-to-run spread - (max - min) / median over its six runs - is what this / parent - 1 is held
against.  Exit status 1 when a workload's |this / parent - 1| exceeds that spread.

  python tools/dispatch_ab.py PARENT.so [--rounds 3] [--cases c2,c1,c4] [--out profiles/dispatch_ab.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"c2": (20, 5), "c1": (40, 5), "c3": (20, 5), "c4": (300, 30), "c4h": (100, 10)}        # workload -> (steps, warm-up)

ap = argparse.ArgumentParser()
ap.add_argument("parent")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--cases", default="c2,c1,c4")
ap.add_argument("--out", default=None)
a = ap.parse_args()
parent = os.path.abspath(a.parent)
if not os.path.exists(parent):
    sys.exit(f"dispatch_ab: {parent} not found (build the parent commit's library with its own build.sh)")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def bench(case, lib):
    env = dict(os.environ)
    env.pop("DFN_LIB", None)
    if lib:
        env["DFN_LIB"] = lib
    steps, warmup = CASES[case]
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--workload", case,
           "--no-cpu-baseline"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    js = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 or len(js) != 1:
        sys.exit(f"dispatch_ab: bench.py failed for {case}:\n{out.stdout[-2000:]}{out.stderr[-4000:]}")
    return json.loads(js[0])["ms_per_step"]


say(f"dispatch_ab: in-tree library against {os.path.basename(parent)}; bench.py --gpus 1, one process per library, workload and round; "
    f"{a.rounds} rounds of (parent, this, parent); medians of ms_per_step")
bad = 0
for case in a.cases.split(","):
    p, t = [], []
    for _ in range(a.rounds):
        p.append(bench(case, parent))
        t.append(bench(case, None))
        p.append(bench(case, parent))
    mp, mt = statistics.median(p), statistics.median(t)
    spread = (max(p) - min(p)) / mp
    inside = abs(mt / mp - 1.0) <= spread
    bad += 0 if inside else 1
    say(f"{case:4s} {CASES[case][0]:4d} steps  parent {mp:8.4f} (" + " ".join(f"{x:.4f}" for x in p) + f")  this {mt:8.4f} ("
        + " ".join(f"{x:.4f}" for x in t) + f")  this / parent {mt / mp:.4f}  parent's own spread {spread * 100:.2f} %  -> "
        + ("inside" if inside else "OUTSIDE"))
if a.out:
    with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(1 if bad else 0)
