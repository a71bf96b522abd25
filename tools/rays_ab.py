#!/usr/bin/env python3
"""Developer tool: the render kernels for caller-supplied rays (dfn_render_rays_fwd) against the plain ones (dfn_render_fwd), on the
same frame, in one process, interleaved.  A C2-shaped frame (450 x 450, 64 + 128 samples) of the synthetic 256-wide decoder, head only
and with two fields; the rays launch is fed the frame's own pinhole rays (engine.get_rays) and its background plate, so the two
launches compute the same image.  A rays kernel reads 24 (one field) to 56 (two fields, with bounds) more bytes per ray and skips
make_ray, against more than 1,000 MFMAs per MLP pass.

Per tier and field count: warm-up of both entry points, then ROUNDS rounds of [plain x REPS frames | rays x REPS frames] timed with
device events; prints the per-round times, their median, and the ratio of the medians (rays / plain).  The RGB of the two launches is
compared bit for bit before anything is timed.

  python tools/rays_ab.py [--tiers f16,f32] [--fields 1,2] [--rounds 3] [--reps 4] [--bounds] [--out profiles/rays_ab.txt]"""
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
ap.add_argument("--fields", default="1,2")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--bounds", action="store_true", help="also pass per-ray bounds (filled with the frame's near / far)")
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
o_h, d_h = engine.get_rays(H, W, sc["focal"], sc["poses"][0], sc["cx"], sc["cy"])
o_t, d_t = engine.get_rays(H, W, sc["focal"], sc["pose_body"], sc["cx"], sc["cy"])
bounds = torch.tensor([sc["near"], sc["far"]], dtype=torch.float32, device=dev).repeat(H * W, 1) if a.bounds else None
lines = [f"rays_ab: {torch.cuda.get_device_name(0)}; synthetic Decoder(hidden_size=256); {H} x {W} rays, 64 + 128 samples; the rays launch "
         f"renders the frame's own pinhole rays{' with per-ray bounds' if a.bounds else ''}; {a.rounds} interleaved rounds x {a.reps} frames "
         "per entry point, device events; ms per frame"]


def say(s):
    print(s, flush=True)
    lines.append(s)


def one(pk, bias, fr, rays):
    if rays is None:
        return engine.render(pk, bias, fr, bg)
    return engine.render(pk, bias, fr, bg, rays=rays, bounds=bounds)


def timed(pk, bias, fr, reps, rays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        one(pk, bias, fr, rays)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for tier in a.tiers.split(","):
    pk = engine.PackedDecoder(flat, tier)
    for fields in [int(f) for f in a.fields.split(",")]:
        shape = "c2 (head only)" if fields == 1 else "c2 (two fields)"
        bias = pk.fold(sig, sigt if fields == 2 else None, zs, za)
        fr = engine.make_frame(H, W, sc["focal"], sc["cx"], sc["cy"], sc["poses"][0], sc["pose_body"], sc["near"], sc["far"], n_fine=128,
                               fields=fields)
        rays = engine.pack_rays(o_h, d_h, *((o_t, d_t) if fields == 2 else ()))
        imgs = {}
        for key, r in (("plain", None), ("rays", rays)):        # warm-up (code objects, clocks) + the frames to compare
            for _ in range(2):
                imgs[key] = one(pk, bias, fr, r)
        torch.cuda.synchronize()
        same = all(torch.equal(x, y) for x, y in zip(imgs["plain"], imgs["rays"]) if x is not None)
        t = {"plain": [], "rays": []}
        for _ in range(a.rounds):
            for key, r in (("plain", None), ("rays", rays)):
                t[key].append(timed(pk, bias, fr, a.reps, r))
        m = {k: statistics.median(v) for k, v in t.items()}
        say(f"{shape:16s} {tier:6s} plain: median {m['plain']:8.3f} (rounds " + " ".join(f"{x:.3f}" for x in t["plain"]) +
            f")  |  rays: median {m['rays']:8.3f} (rounds " + " ".join(f"{x:.3f}" for x in t["rays"]) +
            f")  |  rays / plain = {m['rays'] / m['plain']:.4f}  |  RGB bit-equal: {same}")
        del bias, rays
    del pk
if a.out:
    with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
