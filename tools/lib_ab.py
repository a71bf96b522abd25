#!/usr/bin/env python3
"""Developer tool: interleaved A/B of any number of libraries through bench.py (one bench.py process per library, workload and
round, DFN_LIB selects the library; the libraries take turns inside every round):
  python tools/lib_ab.py --libs parent=exp_libs/parent.so,this --cases c2,c1 --rounds 3 --out profiles/x.txt
The first library is the reference: per library the rounds' ms_per_step, their median, the ratio to the reference (of the medians
and round by round), `roofline.kernel_ms`, the in-kernel clock, and the reference's own round-to-round spread.  A name without a
path is the in-tree library.  A failed bench.py ends the run.
CASES and run_bench() are also what tools/mfma16_ab.py (two libraries, with a verdict per workload) runs on."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {
    "c2": ["--workload", "c2"], "c1": ["--workload", "c1"], "c3": ["--workload", "c3"], "c5": ["--workload", "c5"],
    "c2_512": ["--workload", "c2", "--size", "512"],
    "c2_f32": ["--workload", "c2", "--tier", "f32"], "c2_bf16": ["--workload", "c2", "--tier", "bf16"], "c4": ["--workload", "c4"],
}


def run_bench(case, lib, steps, warmup):
    """one bench.py process on workload `case` with library `lib` (None: the in-tree one) -> {"ms", "kernel_ms", "ghz"};
    RuntimeError with the process's output if it fails"""
    env = dict(os.environ)
    env.pop("DFN_LIB", None)
    if lib:
        env["DFN_LIB"] = lib
    n = steps if case != "c5" else max(2, steps // 8)                   # (a c5 step is eight frames)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(n), "--warmup", str(warmup)] + CASES[case]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    js = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 or len(js) != 1:
        raise RuntimeError(f"bench.py failed for {case} with {lib or 'the in-tree library'}: exit {out.returncode}\n"
                           f"{out.stdout[-2000:]}{out.stderr[-4000:]}")
    r = json.loads(js[0])
    rf = r.get("roofline") or {}
    return {"ms": r["ms_per_step"], "kernel_ms": rf.get("kernel_ms"), "ghz": rf.get("clock_ghz")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True)
    ap.add_argument("--cases", default="c2")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    libs = []
    for item in a.libs.split(","):
        name, _, path = item.partition("=")
        libs.append((name, os.path.join(ROOT, path) if path else None))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(os.path.join(ROOT, a.out), "w") as f:
                f.write("\n".join(lines) + "\n")

    say(f"bench.py --gpus 1 --steps {a.steps} --warmup {a.warmup}; one process per library, workload and round; libraries interleaved "
        f"({', '.join(n for n, _ in libs)}), {a.rounds} rounds")
    for case in a.cases.split(","):
        t = {n: [] for n, _ in libs}
        for _ in range(a.rounds):
            for n, lib in libs:
                try:
                    t[n].append(run_bench(case, lib, a.steps, a.warmup))
                except RuntimeError as e:
                    say(str(e))
                    sys.exit(1)                          # nothing more on the GPU after a failure
        ref = libs[0][0]
        pms = [x["ms"] for x in t[ref]]
        mp = statistics.median(pms)
        spread = (max(pms) - min(pms)) / mp
        for n, _ in libs:
            ms = [x["ms"] for x in t[n]]
            ghz = [x["ghz"] for x in t[n] if x["ghz"] is not None]
            kms = [x["kernel_ms"] for x in t[n] if x["kernel_ms"] is not None]
            per_round = " ".join(f"{m / p:.4f}" for m, p in zip(ms, pms))
            say(f"{case:8s} {n:10s} ms_per_step " + " ".join(f"{x:.3f}" for x in ms) + f"  median {statistics.median(ms):.3f}  / {ref} "
                f"{statistics.median(ms) / mp:.4f} (per round {per_round})  kernel_ms {statistics.median(kms) if kms else float('nan'):.3f}  "
                f"clock {statistics.median(ghz) if ghz else float('nan'):.3f} GHz" + (f"  [{ref}'s spread {spread * 100:.2f} %]" if n == ref else ""))


if __name__ == "__main__":
    main()
