#!/usr/bin/env python3
"""Developer tool: what the ray gradients of the fused training step cost.  The c4-shaped f32 step on caller-supplied rays
(training.render_train(rays=): 2048 rays of the synthetic 256-wide decoder, two fields, forward + backward, MSE on both images, no
optimizer, constant conditioning signals), coarse (64 samples) and hierarchical (64 + 128), once with rays that do not require grad -
the launches of the step as it was - and once with rays that do (dfn_composite_bwd[_hier]_rays_zg in place of _rays_z, then
dfn_points_grad per field and dfn_rays_grad), in one process, interleaved.

Per sample count: warm-up of both forms and a check that every parameter gradient, both signal gradients and both images are bit for bit
the same; then ROUNDS rounds of [without x REPS steps | with x REPS steps] timed with device events: the per-round times, their median,
the spread of the step without ray gradients ((max - min) / median) and the ratio of the medians (with / without).  Then each new
kernel on its own, on the arrays the last step left behind: five batches of REPS back-to-back launches, one device-event pair around
each batch, the median batch's time per launch (one pair around a single launch would measure the events and the launch with a 10-us
kernel).  There is no pass threshold.

  python tools/ray_grad_ab.py [--fine 0,128] [--rays 2048] [--rounds 3] [--reps 20] [--out profiles/ray_grad_ab.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dfa-nerf_amd"))
import torch
from dfanerf import engine, synth, training
from dfanerf._lib import check, lib
from dfanerf.decoder import Decoder

ap = argparse.ArgumentParser()
ap.add_argument("--fine", default="0,128")
ap.add_argument("--rays", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
a = ap.parse_args()

engine.require_gpu()
dev = torch.device("cuda:0")
sc = synth.bench_scene(0, n_frames=2)
st = synth.synth_all_states(0)
zs, za = [torch.from_numpy(v).to(dev) for v in synth.synth_latents(0)]
sig = torch.from_numpy(synth.synth_tensor(0, "g3/sig", (96,), 0.8))[None].to(dev).requires_grad_(True)
sigt = torch.from_numpy(synth.synth_tensor(0, "g3/sigt", (42,), 0.8)).to(dev).requires_grad_(True)
H, W, n = sc["H"], sc["W"], a.rays
pix = ((torch.arange(n, dtype=torch.int64) * 3163) % (H * W)).to(dev)
bg = (torch.from_numpy(sc["bg"]).float() / 255.0).reshape(-1, 3).to(dev)[pix].contiguous()
rays = {False: training.pinhole_rays(sc["poses"][0], sc["pose_body"], pix, H, W, sc["focal"], sc["cx"], sc["cy"])}
rays[True] = rays[False].clone().requires_grad_(True)
tgt = torch.rand(n, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
dec = Decoder(z_dim=256, hidden_size=256, dim_signal=96, use_deformation_field=True)
dec.load_state_dict({k: torch.from_numpy(v) for k, v in st["decoder"].items()})
dec.to(dev)
lines = [f"ray_grad_ab: {torch.cuda.get_device_name(0)}; synthetic Decoder(hidden_size=256); f32 tier; {n} rays, two fields, forward + "
         f"backward on caller-supplied rays (MSE on both images; no optimizer); {a.rounds} interleaved rounds x {a.reps} steps per form, "
         f"device events; ms per step"]


def say(s):
    print(s, flush=True)
    lines.append(s)


def step(buf, fr, grad):
    dec.zero_grad(set_to_none=True)
    sig.grad = sigt.grad = rays[True].grad = None
    rh, rc = training.render_train(dec, buf, fr, bg, None, sig, sigt, zs[0, :2], za[0, :2], rays=rays[grad])
    (((rh - tgt) ** 2).mean() + ((rc - tgt) ** 2).mean()).backward()
    return rh, rc


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for n_fine in [int(f) for f in a.fine.split(",")]:
    shape = "c4 (64)" if n_fine == 0 else f"c4h (64 + {n_fine})"
    buf = training.TrainBuffers("f32", n, dev, n_fine=n_fine)
    fr = engine.make_frame(H, W, sc["focal"], sc["cx"], sc["cy"], sc["poses"][0], sc["pose_body"], sc["near"], sc["far"], ray_count=n,
                           n_fine=n_fine, fields=2)
    keep = {}
    for grad in (False, True):                       # warm-up (code objects, clocks) + the results to compare
        for _ in range(3):
            rh, rc = step(buf, fr, grad)
        torch.cuda.synchronize()
        keep[grad] = [rh.detach().clone(), rc.detach().clone(), sig.grad.clone(), sigt.grad.clone()] + \
                     [p.grad.detach().clone() for p in dec.parameters() if p.grad is not None]
    same = len(keep[False]) == len(keep[True]) > 40 and all(torch.equal(x, y) for x, y in zip(keep[False], keep[True]))
    d_rays = rays[True].grad
    t = {False: [], True: []}
    for _ in range(a.rounds):
        for grad in (False, True):
            t[grad].append(timed(lambda: step(buf, fr, grad), a.reps))
    m = {k: statistics.median(v) for k, v in t.items()}
    spread = (max(t[False]) - min(t[False])) / m[False]
    say(f"{shape:14s} without: median {m[False]:7.3f} (rounds " + " ".join(f"{x:.3f}" for x in t[False]) + f"; spread {spread:.4f})  |  "
        f"with ray gradients: median {m[True]:7.3f} (rounds " + " ".join(f"{x:.3f}" for x in t[True]) +
        f")  |  with / without = {m[True] / m[False]:.4f}  |  images, signal and {len(keep[True]) - 4} parameter gradients bit-equal: {same}"
        f"  |  |d_rays| {float(d_rays.norm()):.3e}, finite: {bool(torch.isfinite(d_rays).all())}")
    # the new kernels on their own, on what the last step (with ray gradients) left in the buffers
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    g, out, dn = buf.g_pts, torch.empty(n, 12, device=dev), buf.d_norm
    dh, dc, ds = torch.randn(n, 3, device=dev), torch.randn(n, 3, device=dev), torch.empty_like(buf.dsamples)
    hier = (p(buf.z_all), p(buf.ranks)) if n_fine else ()
    zname = "dfn_composite_bwd_hier_rays_z" if n_fine else "dfn_composite_bwd_rays_z"
    calls = {
        "points_grad(head)": lambda: check(lib.dfn_points_grad(0, 0, buf.NP, p(buf.flat), p(buf.act[0]), p(buf.dy[0]), p(g[0][0]), p(g[0][1]), s)),
        "points_grad(torso)": lambda: check(lib.dfn_points_grad(0, 1, buf.NP, p(buf.flat), p(buf.act[1]), p(buf.dy[1]), p(g[1][0]), p(g[1][1]), s)),
        "rays_grad": lambda: check(lib.dfn_rays_grad(0, C.byref(fr), p(rays[False]), None, p(buf.z_all), p(buf.ranks), p(g[0][0]), p(g[0][1]),
                                                     p(g[1][0]), p(g[1][1]), p(dn), p(out), s)),
        "composite_bwd _z": lambda: check(getattr(lib, zname)(C.byref(fr), p(rays[False]), None, p(bg), None, p(buf.samples), *hier, p(dh),
                                                               p(dc), p(ds), None, 0, s)),
        "composite_bwd _zg": lambda: check(getattr(lib, zname + "g")(C.byref(fr), p(rays[False]), None, p(bg), None, p(buf.samples), *hier,
                                                                      p(dh), p(dc), p(ds), None, 0, p(dn), s)),
    }
    for name, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        us = statistics.median(timed(fn, a.reps) for _ in range(5)) * 1000.0
        say(f"{shape:14s}   {name:20s} {us:8.1f} us per launch (median of 5 batches of {a.reps} back-to-back launches)")
    del buf
if a.out:
    with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
