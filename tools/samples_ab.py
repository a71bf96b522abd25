#!/usr/bin/env python3
"""Developer tool: what the hierarchical mode's sample counts cost and buy.  The synthetic 256-wide decoder on a C2 / C3-shaped frame
(450 x 450; C2 = head only, C3 = two fields), rendered at (n_coarse, n_fine) = 32+32, 32+64, 64+32, 64+64 and 64+128.

  1. cost of the knob: per tier (f16, f32) and shape, ROUNDS rounds of [pair x REPS frames] for every pair, interleaved, timed with
     device events; prints ms per frame (median of the rounds), frames/s, and the time relative to 64+128 divided by the decoder
     evaluation count relative to 64+128, (n_coarse + n_fine) / 192.  Exit status 1 if a new pair is not faster than 64+128.
  2. what the knob costs in the image: PSNR of every pair's f32 render against the 64+128 f32 render of the same frame.  (The
     synthetic scene says little about a trained head: orientation only.)
  3. --regress PARENT.so: no regression where nothing was asked to change.  64+128 and 64+64 for C2 f16, C3 f16 and C2 f32 with the
     in-tree library against the library given (one built from the parent commit: tools/build_variant.sh), each measurement in a
     process of its own (DFN_LIB selects the library), the two libraries interleaved, ROUNDS rounds; prints the ratio of the medians
     and the round-to-round spread of the parent's own rounds, (max - min) / median.

  python tools/samples_ab.py [--rounds 3] [--reps 4] [--out profiles/samples_ab.txt]
  python tools/samples_ab.py --regress exp_libs/parent.so [--out profiles/samples_ab_regress.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dfa-nerf_amd"))

PAIRS = [(32, 32), (32, 64), (64, 32), (64, 64), (64, 128)]
NEW = PAIRS[:3]
REGRESS = [("f16", 1), ("f16", 2), ("f32", 1)]           # C2 f16, C3 f16, C2 f32
REGRESS_PAIRS = [(64, 128), (64, 64)]

ap = argparse.ArgumentParser()
ap.add_argument("--tiers", default="f16,f32")
ap.add_argument("--fields", default="1,2")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--regress", metavar="PARENT.so", default=None)
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)      # internal: one measurement process of --regress
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def finish(status=0):
    if a.out:
        with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(status)


def shape_name(fields):
    return "c2 (head only)" if fields == 1 else "c3 (two fields)"


if a.regress and not a.child:
    parent = a.regress if os.path.isabs(a.regress) else os.path.join(ROOT, a.regress)
    if not os.path.exists(parent):
        sys.exit(f"samples_ab: {parent} not found (build the parent commit's library, e.g. with tools/build_variant.sh in a checkout of it)")
    t = {}
    say(f"samples_ab --regress: in-tree library against {os.path.relpath(parent, ROOT)}; 450 x 450, synthetic Decoder(hidden_size=256); one "
        f"process per library and round, interleaved, {a.rounds} rounds x {a.reps} frames, device events; ms per frame")
    for r in range(a.rounds):
        for name, lib in (("parent", parent), ("this", None)):
            env = dict(os.environ)
            env.pop("DFN_LIB", None)
            if lib:
                env["DFN_LIB"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)], env=env, capture_output=True,
                                 text=True, timeout=600)
            if out.returncode != 0:
                sys.exit(f"samples_ab: the {name} measurement failed:\n{out.stdout[-2000:]}{out.stderr[-4000:]}")
            if r == 0:
                say(f"  {name}: {json.loads(out.stdout.strip().splitlines()[-1])['version']}")
            for k, ms in json.loads(out.stdout.strip().splitlines()[-1])["ms"].items():
                t.setdefault(k, {}).setdefault(name, []).append(ms)
    worst = 0
    for k, v in t.items():
        mp, mt = statistics.median(v["parent"]), statistics.median(v["this"])
        spread = (max(v["parent"]) - min(v["parent"])) / mp
        inside = abs(mt / mp - 1.0) <= spread
        worst += 0 if inside or mt <= mp else 1
        say(f"{k:28s} parent: median {mp:8.3f} (rounds " + " ".join(f"{x:.3f}" for x in v["parent"]) + f")  |  this: median {mt:8.3f} (rounds "
            + " ".join(f"{x:.3f}" for x in v["this"]) + f")  |  this / parent = {mt / mp:.4f}  |  parent's round-to-round spread {spread * 100:.2f} %"
            + ("" if inside else ("  |  OUTSIDE the spread (faster)" if mt <= mp else "  |  OUTSIDE the spread (SLOWER)")))
    finish(1 if worst else 0)

import torch
from dfanerf import _lib, engine, synth

engine.require_gpu()
dev = torch.device("cuda:0")
sc = synth.bench_scene(0, n_frames=2)
flat = engine.flatten_state(synth.synth_all_states(0)["decoder"], dev)
zs, za = [torch.from_numpy(v).to(dev)[0] for v in synth.synth_latents(0)]
sig = torch.from_numpy(synth.synth_tensor(0, "g3/sig", (96,), 0.8)).to(dev)
sigt = torch.from_numpy(synth.synth_tensor(0, "g3/sigt", (42,), 0.8)).to(dev)
bg = (torch.from_numpy(sc["bg"]).float() / 255.0).reshape(-1, 3).to(dev)
H, W = sc["H"], sc["W"]


def frame(nc, nf, fields):
    return engine.make_frame(H, W, sc["focal"], sc["cx"], sc["cy"], sc["poses"][0], sc["pose_body"], sc["near"], sc["far"], n_coarse=nc,
                             n_fine=nf, fields=fields)


def timed(pk, bias, fr, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        engine.render(pk, bias, fr, bg)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


if a.child:                 # one library, one round: the frames of --regress
    ms = {}
    for tier, fields in REGRESS:
        pk = engine.PackedDecoder(flat, tier)
        bias = pk.fold(sig, sigt if fields == 2 else None, zs, za)
        frs = {p: frame(*p, fields) for p in REGRESS_PAIRS}
        for fr in frs.values():
            for _ in range(2):
                engine.render(pk, bias, fr, bg)
        torch.cuda.synchronize()
        for p, fr in frs.items():
            ms[f"{shape_name(fields)} {tier} {p[0]}+{p[1]}"] = timed(pk, bias, fr, a.reps)
        del pk, bias
    print(json.dumps({"version": _lib.lib.dfn_version().decode(), "ms": ms}))
    sys.exit(0)

say(f"samples_ab: {torch.cuda.get_device_name(0)}; synthetic Decoder(hidden_size=256); {H} x {W} rays; the hierarchical mode at "
    + ", ".join(f"{c}+{f}" for c, f in PAIRS) + f" samples; {a.rounds} interleaved rounds x {a.reps} frames per pair, device events; ms per "
    "frame; evals = (n_coarse + n_fine) / 192, the decoder evaluations per ray and field relative to 64+128")
slower = []
for tier in a.tiers.split(","):
    pk = engine.PackedDecoder(flat, tier)
    for fields in [int(f) for f in a.fields.split(",")]:
        bias = pk.fold(sig, sigt if fields == 2 else None, zs, za)
        frs = {p: frame(*p, fields) for p in PAIRS}
        for fr in frs.values():                                  # warm-up (code objects, clocks)
            for _ in range(2):
                engine.render(pk, bias, fr, bg)
        torch.cuda.synchronize()
        t = {p: [] for p in PAIRS}
        for _ in range(a.rounds):
            for p in PAIRS:
                t[p].append(timed(pk, bias, frs[p], a.reps))
        m = {p: statistics.median(v) for p, v in t.items()}
        full = m[(64, 128)]
        for p in PAIRS:
            ev = (p[0] + p[1]) / 192.0
            say(f"{shape_name(fields):16s} {tier:4s} {p[0]:3d}+{p[1]:<3d}  median {m[p]:8.3f} ms  {1000.0 / m[p]:6.2f} frames/s  (rounds "
                + " ".join(f"{x:.3f}" for x in t[p]) + f")  |  time / 64+128 = {m[p] / full:.4f}  evals = {ev:.4f}  time per eval = {m[p] / full / ev:.4f}")
            if p in NEW and not m[p] < full:
                slower.append((tier, fields, p))
        if tier == "f16" and fields == 2:
            say(f"    c3 f16 at 32+64: {m[(32, 64)]:.2f} ms per frame - " + ("under" if m[(32, 64)] < 40.0 else "NOT under") + " the 40 ms of 25 frames/s")
        del bias
    del pk
# ---- the image: every pair's f32 render against the 64+128 f32 render
pk = engine.PackedDecoder(flat, "f32")
say("image (synthetic frame, f32 tier): PSNR of each pair's render against the 64+128 render of the same frame - the synthetic scene "
    "says little about a trained head: orientation only")
for fields in (1, 2):
    bias = pk.fold(sig, sigt if fields == 2 else None, zs, za)
    ref = engine.render(pk, bias, frame(64, 128, fields), bg)[fields - 1].double()
    row = []
    for p in PAIRS[:-1]:
        img = engine.render(pk, bias, frame(*p, fields), bg)[fields - 1].double()
        mse = float(((img - ref) ** 2).mean())
        row.append(f"{p[0]}+{p[1]}: {99.0 if mse == 0 else -10.0 * torch.log10(torch.tensor(mse)).item():.2f} dB")
    say(f"    {shape_name(fields):16s} " + "   ".join(row))
for tier, fields, p in slower:
    say(f"NOT FASTER than 64+128: {shape_name(fields)} {tier} {p[0]}+{p[1]}")
finish(1 if slower else 0)
