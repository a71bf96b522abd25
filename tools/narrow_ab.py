#!/usr/bin/env python3
"""Developer tool: the native 128-wide inference program against the padded 256-wide one, on the SAME 128-wide network, in one
process, interleaved.  A C2-shaped frame (450 x 450, 64 + 128 samples, head only) and a C3-shaped one (two fields) of the synthetic
Decoder(hidden_size=128, z_dim=64) - golden G18's network.  The yardstick is the padded program: it is what such a decoder ran
before the 128-wide program existed, and what DFN_WIDTH=256 still selects.

Per (workload, tier): warm-up of both packs, then ROUNDS rounds of [padded x REPS frames | native x REPS frames] timed with device
events; prints the per-round times, their median and spread, and the ratio of the medians.  The frames of the two programs are
compared bit for bit before anything is timed (faster and different is not faster).

  python tools/narrow_ab.py [--tiers f16,f16x3,f32] [--rounds 3] [--reps 6] [--out profiles/narrow_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dfa-nerf_amd"))
import torch
from dfanerf import engine, synth

ap = argparse.ArgumentParser()
ap.add_argument("--tiers", default="f16,f16x3,f32")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--out", default=None)
a = ap.parse_args()

engine.require_gpu()
dev = torch.device("cuda:0")
sc = synth.bench_scene(0, n_frames=2)
flat = engine.flatten_state(synth.synth_decoder_state(0, z_dim=64, hidden=128), dev)
zs, za = [torch.from_numpy(v).to(dev)[0] for v in synth.synth_latents(0, z_dim=64)]
sig = torch.from_numpy(synth.synth_tensor(0, "g3/sig", (96,), 0.8)).to(dev)
sigt = torch.from_numpy(synth.synth_tensor(0, "g3/sigt", (42,), 0.8)).to(dev)
bg = (torch.from_numpy(sc["bg"]).float() / 255.0).reshape(-1, 3).to(dev)
H, W = sc["H"], sc["W"]
lines = [f"narrow_ab: {torch.cuda.get_device_name(0)}; synthetic Decoder(hidden_size=128, z_dim=64); {H} x {W} rays, 64 + 128 samples; "
         f"{a.rounds} interleaved rounds x {a.reps} frames per program, device events; ms per frame"]


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(pk, bias, fr, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        engine.render(pk, bias, fr, bg)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for wl, fields in (("c2 (head only)", 1), ("c3 (two fields)", 2)):
    for tier in a.tiers.split(","):
        pks = {w: engine.PackedDecoder(flat, tier, fields=(0, 1), z_dim=64, width=w) for w in (256, 128)}
        bias = {w: pk.fold(sig, sigt if fields == 2 else None, zs, za) for w, pk in pks.items()}
        fr = engine.make_frame(H, W, sc["focal"], sc["cx"], sc["cy"], sc["poses"][0], sc["pose_body"], sc["near"], sc["far"],
                               n_fine=128, fields=fields)
        imgs = {}
        for w, pk in pks.items():                   # warm-up (code objects, clocks) + the frames to compare
            for _ in range(2):
                imgs[w] = engine.render(pk, bias[w], fr, bg)
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) for x, y in zip(imgs[256], imgs[128]) if x is not None)
        t = {256: [], 128: []}
        for _ in range(a.rounds):
            for w in (256, 128):
                t[w].append(timed(pks[w], bias[w], fr, a.reps))
        m = {w: statistics.median(v) for w, v in t.items()}
        say(f"{wl:16s} {tier:6s} padded 256: median {m[256]:8.3f} (rounds " + " ".join(f"{x:.3f}" for x in t[256]) + f")  |  native 128: "
            f"median {m[128]:8.3f} (rounds " + " ".join(f"{x:.3f}" for x in t[128]) + f")  |  padded / native = {m[256] / m[128]:.2f}x  |  "
            f"frames bit-equal: {same}")
        del pks, bias
if a.out:
    with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
