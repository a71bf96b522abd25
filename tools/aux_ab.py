#!/usr/bin/env python3
"""Developer tool: the aux render kernels (dfn_render_fwd_aux: opacity and expected depth next to the RGB) against the plain ones
(dfn_render_fwd), on the same frame, in one process, interleaved.  A C2-shaped frame (450 x 450, 64 + 128 samples, head only) of the
synthetic 256-wide decoder; --fields 2 for the C3 shape.  The extra work of an aux kernel is two 5-step butterflies per 32-sample
tile and image and two scalar additions, against more than 1,000 MFMAs per MLP pass.

Per tier: warm-up of both entry points, then ROUNDS rounds of [plain x REPS frames | aux x REPS frames] timed with device events;
prints the per-round times, their median, and the ratio of the medians (aux / plain).  The RGB of the two launches is compared bit
for bit before anything is timed.

  python tools/aux_ab.py [--tiers f16,f32] [--fields 1] [--rounds 3] [--reps 4] [--out profiles/aux_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dfa-nerf_amd"))
import torch
from dfanerf import engine, synth

ap = argparse.ArgumentParser()
ap.add_argument("--tiers", default="f16,f32")
ap.add_argument("--fields", type=int, default=1)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--out", default=None)
a = ap.parse_args()

engine.require_gpu()
dev = torch.device("cuda:0")
sc = synth.bench_scene(0, n_frames=2)
flat = engine.flatten_state(synth.synth_all_states(0)["decoder"], dev)
zs, za = [torch.from_numpy(v).to(dev)[0] for v in synth.synth_latents(0)]
sig = torch.from_numpy(synth.synth_tensor(0, "g3/sig", (96,), 0.8)).to(dev)
sigt = torch.from_numpy(synth.synth_tensor(0, "g3/sigt", (42,), 0.8)).to(dev)
bg = (torch.from_numpy(sc["bg"]).float() / 255.0).reshape(-1, 3).to(dev)
H, W = sc["H"], sc["W"]
shape = "c2 (head only)" if a.fields == 1 else "c3 (two fields)"
lines = [f"aux_ab: {torch.cuda.get_device_name(0)}; synthetic Decoder(hidden_size=256); {shape}; {H} x {W} rays, 64 + 128 samples; "
         f"{a.rounds} interleaved rounds x {a.reps} frames per entry point, device events; ms per frame"]


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(pk, bias, fr, reps, aux):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        engine.render(pk, bias, fr, bg, want_aux=aux)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for tier in a.tiers.split(","):
    pk = engine.PackedDecoder(flat, tier)
    bias = pk.fold(sig, sigt if a.fields == 2 else None, zs, za)
    fr = engine.make_frame(H, W, sc["focal"], sc["cx"], sc["cy"], sc["poses"][0], sc["pose_body"], sc["near"], sc["far"], n_fine=128,
                           fields=a.fields)
    imgs = {}
    for aux in (False, True):                       # warm-up (code objects, clocks) + the frames to compare
        for _ in range(2):
            imgs[aux] = engine.render(pk, bias, fr, bg, want_aux=aux)
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(imgs[False][:2], imgs[True][:2]) if x is not None)
    acc = imgs[True][2][:, 0]
    t = {False: [], True: []}
    for _ in range(a.rounds):
        for aux in (False, True):
            t[aux].append(timed(pk, bias, fr, a.reps, aux))
    m = {k: statistics.median(v) for k, v in t.items()}
    say(f"{shape:16s} {tier:6s} plain: median {m[False]:8.3f} (rounds " + " ".join(f"{x:.3f}" for x in t[False]) + f")  |  aux: median "
        f"{m[True]:8.3f} (rounds " + " ".join(f"{x:.3f}" for x in t[True]) + f")  |  aux / plain = {m[True] / m[False]:.4f}  |  RGB bit-equal: "
        f"{same}  |  head opacity in [{float(acc.min()):.3f}, {float(acc.max()):.3f}]")
    del pk, bias
if a.out:
    with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
