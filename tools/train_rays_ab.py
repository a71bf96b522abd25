#!/usr/bin/env python3
"""Developer tool: the fused training step on caller-supplied rays (training.render_train(rays=): dfn_train_rays_fwd[_hier] +
dfn_composite_bwd[_hier]_rays_z) against the plain step (pixel ids), in one process, interleaved.  The c4-shaped step: 2048 rays of the
synthetic 256-wide decoder, two fields, forward + backward of the decoder (MSE on both images, no optimizer, constant conditioning
signals), in the bf16 and the f32 tier, coarse (64 samples) and hierarchical (64 + 128).  The rays step is fed the frame's own pinhole
rays (engine.get_rays) gathered at the plain step's pixels, and that pixels' background rows, so the two steps compute the same
numbers: images and one gradient tensor are compared bit for bit before anything is timed.  A rays kernel reads 48 (with bounds: 56)
more bytes per ray and skips make_ray, against more than 2,000 MFMAs per ray and tile.

Per tier and sample count: warm-up of both forms, then ROUNDS rounds of [plain x REPS steps | rays x REPS steps] timed with device
events; prints the per-round times, their median, the plain step's own round-to-round spread ((max - min) / median) and the ratio of
the medians (rays / plain).  There is no pass threshold.

  python tools/train_rays_ab.py [--tiers bf16,f32] [--fine 0,128] [--rounds 3] [--reps 20] [--bounds] [--out profiles/train_rays_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dfa-nerf_amd"))
import torch
from dfanerf import engine, synth, training
from dfanerf.decoder import Decoder

ap = argparse.ArgumentParser()
ap.add_argument("--tiers", default="bf16,f32")
ap.add_argument("--fine", default="0,128")
ap.add_argument("--rays", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--bounds", action="store_true", help="also pass per-ray bounds (filled with the frame's near / far)")
ap.add_argument("--out", default=None)
a = ap.parse_args()

engine.require_gpu()
dev = torch.device("cuda:0")
sc = synth.bench_scene(0, n_frames=2)
st = synth.synth_all_states(0)
zs, za = [torch.from_numpy(v).to(dev) for v in synth.synth_latents(0)]
sig = torch.from_numpy(synth.synth_tensor(0, "g3/sig", (96,), 0.8))[None].to(dev)
sigt = torch.from_numpy(synth.synth_tensor(0, "g3/sigt", (42,), 0.8)).to(dev)
H, W, n = sc["H"], sc["W"], a.rays
bg_all = (torch.from_numpy(sc["bg"]).float() / 255.0).reshape(-1, 3).to(dev)
pix = ((torch.arange(n, dtype=torch.int64) * 3163) % (H * W)).to(dev)
pix32 = pix.to(torch.int32)
o_h, d_h = engine.get_rays(H, W, sc["focal"], sc["poses"][0], sc["cx"], sc["cy"])
o_t, d_t = engine.get_rays(H, W, sc["focal"], sc["pose_body"], sc["cx"], sc["cy"])
rays = engine.pack_rays(*(x.reshape(-1, 3)[pix] for x in (o_h, d_h, o_t, d_t)))
bg_rays = bg_all[pix].contiguous()
bounds = torch.tensor([sc["near"], sc["far"]], dtype=torch.float32, device=dev).repeat(n, 1) if a.bounds else None
tgt = torch.rand(n, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
dec = Decoder(z_dim=256, hidden_size=256, dim_signal=96, use_deformation_field=True)
dec.load_state_dict({k: torch.from_numpy(v) for k, v in st["decoder"].items()})
dec.to(dev)
lines = [f"train_rays_ab: {torch.cuda.get_device_name(0)}; synthetic Decoder(hidden_size=256); {n} rays, two fields, forward + backward "
         f"(MSE on both images; no optimizer); the rays step trains on the frame's own pinhole rays"
         f"{' with per-ray bounds' if a.bounds else ''}; {a.rounds} interleaved rounds x {a.reps} steps per form, device events; ms per step"]


def say(s):
    print(s, flush=True)
    lines.append(s)


def step(buf, fr, use_rays):
    dec.zero_grad(set_to_none=True)
    if use_rays:
        rh, rc = training.render_train(dec, buf, fr, bg_rays, None, sig, sigt, zs[0, :2], za[0, :2], rays=rays, bounds=bounds)
    else:
        rh, rc = training.render_train(dec, buf, fr, bg_all, pix32, sig, sigt, zs[0, :2], za[0, :2])
    (((rh - tgt) ** 2).mean() + ((rc - tgt) ** 2).mean()).backward()
    return rh, rc


def timed(buf, fr, reps, use_rays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        step(buf, fr, use_rays)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for tier in a.tiers.split(","):
    for n_fine in [int(f) for f in a.fine.split(",")]:
        shape = "c4 (64)" if n_fine == 0 else f"c4h (64 + {n_fine})"
        buf = training.TrainBuffers(tier, n, dev, n_fine=n_fine)
        fr = engine.make_frame(H, W, sc["focal"], sc["cx"], sc["cy"], sc["poses"][0], sc["pose_body"], sc["near"], sc["far"], ray_count=n,
                               n_fine=n_fine, fields=2)
        keep = {}
        for key in ("plain", "rays"):                    # warm-up (code objects, clocks) + the results to compare
            for _ in range(3):
                rh, rc = step(buf, fr, key == "rays")
            torch.cuda.synchronize()
            keep[key] = (rh.detach().clone(), rc.detach().clone(), dec.blocks[3].weight.grad.detach().clone())
        same = all(torch.equal(x, y) for x, y in zip(keep["plain"], keep["rays"]))
        t = {"plain": [], "rays": []}
        for _ in range(a.rounds):
            for key in ("plain", "rays"):
                t[key].append(timed(buf, fr, a.reps, key == "rays"))
        m = {k: statistics.median(v) for k, v in t.items()}
        spread = (max(t["plain"]) - min(t["plain"])) / m["plain"]
        say(f"{shape:14s} {tier:5s} plain: median {m['plain']:7.3f} (rounds " + " ".join(f"{x:.3f}" for x in t["plain"]) +
            f"; spread {spread:.4f})  |  rays: median {m['rays']:7.3f} (rounds " + " ".join(f"{x:.3f}" for x in t["rays"]) +
            f")  |  rays / plain = {m['rays'] / m['plain']:.4f}  |  images and d blocks.3.weight bit-equal: {same}")
        del buf
if a.out:
    with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
