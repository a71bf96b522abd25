#!/usr/bin/env python3
"""Developer tool: what the two-launch hierarchical render (engine.render_two_pass) costs and buys.  The synthetic
256-wide decoder on a C2 / C3-shaped frame (450 x 450; C2 = head only, C3 = two fields) at 64+128 and 32+64 samples.  Per shape and
pair, ROUNDS interleaved rounds of REPS frames each, timed with device events, of

  f16        one launch, the f16 tier (what bench.py reports)
  two-pass   f16 at the f16x3 tier's fine depths: the total, and its three launches on their own - pass A (the n_coarse-sample f16x3
             coarse pass with its weights), the sampler (dfn_fine_depths), pass B (the n_coarse + n_fine-sample f16 z launch)
  f16x3      one launch, the f16x3 tier
  f32        one launch, the f32 tier

and the PSNR of each image against the f32 frame.  The two-launch route earns its place if its total is below the f16x3 one-launch
frame by more than the round-to-round spread of the f16x3 rows; the ratio is printed either way.

  python tools/twopass_ab.py [--rounds 3] [--reps 2] [--out profiles/twopass_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dfa-nerf_amd"))

PAIRS = [(64, 128), (32, 64)]

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--sampler", default="f16x3")
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


import torch
from dfanerf import engine, synth

engine.require_gpu()
dev = torch.device("cuda:0")
sc = synth.bench_scene(0, n_frames=2)
flat = engine.flatten_state(synth.synth_all_states(0)["decoder"], dev)
zs, za = [torch.from_numpy(v).to(dev)[0] for v in synth.synth_latents(0)]
sig = torch.from_numpy(synth.synth_tensor(0, "g3/sig", (96,), 0.8)).to(dev)
sigt = torch.from_numpy(synth.synth_tensor(0, "g3/sigt", (42,), 0.8)).to(dev)
bg = (torch.from_numpy(sc["bg"]).float() / 255.0).reshape(-1, 3).to(dev)
H, W = sc["H"], sc["W"]
pk = {tier: engine.PackedDecoder(flat, tier) for tier in ("f16", a.sampler, "f16x3", "f32")}


def frame(nc, nf, fields):
    return engine.make_frame(H, W, sc["focal"], sc["cx"], sc["cy"], sc["poses"][0], sc["pose_body"], sc["near"], sc["far"], n_coarse=nc,
                             n_fine=nf, fields=fields)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def psnr(img, ref):
    mse = float(((img.double() - ref.double()) ** 2).mean())
    return 99.0 if mse == 0 else -10.0 * torch.log10(torch.tensor(mse)).item()


say(f"twopass_ab: {torch.cuda.get_device_name(0)}; synthetic Decoder(hidden_size=256); {H} x {W} rays; sampler tier {a.sampler}; "
    f"{a.rounds} interleaved rounds x {a.reps} frames, device events; ms per frame (median of the rounds); PSNR against the f32 frame of "
    "the image the shape ends in (head image for c2, composite for c3)")
for fields in (1, 2):
    shape = "c2 (head only)" if fields == 1 else "c3 (two fields)"
    bias = {tier: p.fold(sig, sigt if fields == 2 else None, zs, za) for tier, p in pk.items()}
    for nc, nf in PAIRS:
        fr, fr_a, fr_b = frame(nc, nf, fields), frame(nc, 0, fields), frame(nc + nf, 0, fields)
        w = engine.render(pk[a.sampler], bias[a.sampler], fr_a, bg, want_weights=True)[3 if fields == 2 else 2]
        z = engine.fine_depths(fr, w)
        rgb = [torch.empty(H * W, 3, device=dev) for _ in range(2)]
        ws = engine.two_pass_workspace(pk["f16"], fr)
        runs = {
            "f16 one launch": lambda: engine.render(pk["f16"], bias["f16"], fr, bg, out_head=rgb[0], out_com=rgb[1] if fields == 2 else None),
            "two-pass total": lambda: engine.render_two_pass(pk[a.sampler], bias[a.sampler], pk["f16"], bias["f16"], fr, bg, out_head=rgb[0],
                                                             out_com=rgb[1] if fields == 2 else None, workspace=ws),
            "  pass A": lambda: engine.render(pk[a.sampler], bias[a.sampler], fr_a, bg, want_weights=True, out_head=rgb[0],
                                              out_com=rgb[1] if fields == 2 else None),
            "  sampler": lambda: engine.fine_depths(fr, w, out=z),
            "  pass B": lambda: engine.render(pk["f16"], bias["f16"], fr_b, bg, z_vals=z, out_head=rgb[0], out_com=rgb[1] if fields == 2 else None),
            "f16x3 one launch": lambda: engine.render(pk["f16x3"], bias["f16x3"], fr, bg, out_head=rgb[0], out_com=rgb[1] if fields == 2 else None),
            "f32 one launch": lambda: engine.render(pk["f32"], bias["f32"], fr, bg, out_head=rgb[0], out_com=rgb[1] if fields == 2 else None),
        }
        for fn in runs.values():                                 # warm-up (code objects, clocks)
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k].append(timed(fn, a.reps))
        m = {k: statistics.median(v) for k, v in t.items()}
        ref = engine.render(pk["f32"], bias["f32"], fr, bg)[fields - 1].clone()
        img = {"f16 one launch": engine.render(pk["f16"], bias["f16"], fr, bg)[fields - 1].clone(),
               "two-pass total": engine.render_two_pass(pk[a.sampler], bias[a.sampler], pk["f16"], bias["f16"], fr, bg)[fields - 1].clone(),
               "f16x3 one launch": engine.render(pk["f16x3"], bias["f16x3"], fr, bg)[fields - 1].clone()}
        for k in runs:
            say(f"{shape:16s} {nc:3d}+{nf:<3d} {k:18s} median {m[k]:8.3f} ms  (rounds " + " ".join(f"{x:.3f}" for x in t[k]) + ")"
                + (f"  |  {psnr(img[k], ref):6.2f} dB against f32" if k in img else ""))
        x3 = t["f16x3 one launch"]
        spread = (max(x3) - min(x3)) / m["f16x3 one launch"]
        gain = 1.0 - m["two-pass total"] / m["f16x3 one launch"]
        say(f"    two-pass / f16x3 = {m['two-pass total'] / m['f16x3 one launch']:.4f}, two-pass / f16 = "
            f"{m['two-pass total'] / m['f16 one launch']:.4f}, f32 / two-pass = {m['f32 one launch'] / m['two-pass total']:.2f}; the f16x3 "
            f"rows' round-to-round spread {spread * 100:.2f} %: the two-launch route is "
            + ("BELOW the f16x3 frame by more than that" if gain > spread else "NOT below the f16x3 frame by more than that"))
if a.out:
    with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
        f.write("\n".join(lines) + "\n")
