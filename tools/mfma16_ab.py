#!/usr/bin/env python3
"""A/B of the f16 tier's MFMA shape (16x16x32, LABNOTES.md 4.7): the in-tree library against one built from the parent commit, through
bench.py itself - what the driver's single line shows.  One bench.py process per library, workload and round (DFN_LIB selects the
library), the two libraries interleaved; per workload the medians of `ms_per_step` and `roofline.kernel_ms`, their ratio, the
in-kernel clock, and the parent's own round-to-round spread: a change counts when it is at least ten times that spread (the
workloads that ride the changed code) or stays inside it (those that must not move).

  python tools/mfma16_ab.py PARENT.so [--rounds 3] [--steps 20] [--warmup 5] [--cases c2,c3,...] [--out profiles/mfma16_ab.txt]
Cases: c2 c1 c3 c5 c2_512 (f16: changed), c2_f32 c2_bf16 c4 (must not move)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from lib_ab import CASES, run_bench                 # noqa: E402  (the workload table and the bench.py runner, shared)

CHANGED = ("c2", "c1", "c3", "c5", "c2_512")

ap = argparse.ArgumentParser()
ap.add_argument("parent")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--cases", default="c2,c1,c3,c5,c2_512,c2_f32,c2_bf16,c4")
ap.add_argument("--out", default=None)
a = ap.parse_args()
parent = a.parent if os.path.isabs(a.parent) else os.path.join(ROOT, a.parent)
if not os.path.exists(parent):
    sys.exit(f"mfma16_ab: {parent} not found (build the parent commit's library, e.g. with tools/build_variant.sh in a checkout of it)")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def bench(case, lib):
    try:
        return run_bench(case, lib, a.steps, a.warmup)
    except RuntimeError as e:
        sys.exit(f"mfma16_ab: {e}")


say(f"mfma16_ab: in-tree library against {os.path.basename(parent)}; bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}, one process per "
    f"library, workload and round, interleaved, {a.rounds} rounds; medians")
bad = 0
for case in a.cases.split(","):
    t = {"parent": [], "this": []}
    for _ in range(a.rounds):
        for name, lib in (("parent", parent), ("this", None)):
            t[name].append(bench(case, lib))

    def med(name, key):
        v = [x[key] for x in t[name] if x[key] is not None]
        return statistics.median(v) if v else float("nan")
    mp, mt = med("parent", "ms"), med("this", "ms")
    pms = [x["ms"] for x in t["parent"]]
    spread = (max(pms) - min(pms)) / mp
    gain = 1.0 - mt / mp
    if case in CHANGED:
        verdict = "gain >= 10 x spread" if gain >= 10.0 * spread else "gain BELOW 10 x the parent's spread"
        bad += 0 if gain >= 10.0 * spread else 1
    else:
        inside = abs(gain) <= spread or mt <= mp
        verdict = "inside the parent's spread (or faster)" if inside else "OUTSIDE the parent's spread (SLOWER)"
        bad += 0 if inside else 1
    say(f"{case:8s} ms_per_step  parent {mp:9.3f} (" + " ".join(f"{x:.3f}" for x in pms) + f")  this {mt:9.3f} ("
        + " ".join(f"{x['ms']:.3f}" for x in t["this"]) + f")  this / parent {mt / mp:.4f}  parent's spread {spread * 100:.2f} %  -> {verdict}")
    say(f"{'':8s} kernel_ms    parent {med('parent', 'kernel_ms'):9.3f}  this {med('this', 'kernel_ms'):9.3f}  ratio "
        f"{med('this', 'kernel_ms') / med('parent', 'kernel_ms'):.4f}   clock GHz  parent {med('parent', 'ghz'):.3f}  this {med('this', 'ghz'):.3f}")
if a.out:
    with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(1 if bad else 0)
