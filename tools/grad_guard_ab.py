#!/usr/bin/env python3
"""Developer tool: what optim.HipAdam's gradient guard costs in the training step.  The c4-shaped step: 2048 rays of the synthetic
256-wide decoder, two fields, forward + backward of the decoder (MSE on both images, constant conditioning signals) and the decoder's
optimizer step - unguarded (`off`: dfn_adam_multi, the launches of the step as it was), with the non-finite skip (`guard`:
dfn_grad_stats' two launches + dfn_adam_multi_guarded) and with the skip plus a norm bound that never binds (`clip`, max_grad_norm
1e9) - in the bf16 and the f32 tier, coarse (64 samples) and hierarchical (64 + 128).

Three decoders with the same weights, one per mode, each with its own optimizer, in one process.  First every mode takes the same
warm-up steps and the parameters of the three are compared bit for bit (nothing triggers: the guarded update is the plain one);
then ROUNDS rounds of [off x REPS | guard x REPS | clip x REPS] are timed with device events.  Printed per shape and tier: the
per-round times, their medians, the off rows' own round-to-round spread ((max - min) / median) and the ratios guard / off and
clip / off.  There is no pass threshold.

Each (tier, sample count) runs in a child process of its own under a time limit; the first child that fails ends the run.

  python tools/grad_guard_ab.py [--tiers bf16,f32] [--fine 0,128] [--rounds 3] [--reps 20] [--limit 180] [--out profiles/grad_guard_ab.txt]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dfa-nerf_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--tiers", default="bf16,f32")
ap.add_argument("--fine", default="0,128")
ap.add_argument("--rays", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--limit", type=int, default=180, help="seconds a child process may take")
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help="(internal) tier:n_fine of the one configuration this process measures")
a = ap.parse_args()

MODES = (("off", {}), ("guard", {"skip_nonfinite": True}), ("clip", {"skip_nonfinite": True, "max_grad_norm": 1e9}))


def child(tier, n_fine):
    import torch
    from dfanerf import engine, synth, training
    from dfanerf.decoder import Decoder
    from dfanerf.optim import HipAdam
    engine.require_gpu()
    dev = torch.device("cuda:0")
    sc = synth.bench_scene(0, n_frames=2)
    st = synth.synth_all_states(0)
    zs, za = [torch.from_numpy(v).to(dev) for v in synth.synth_latents(0)]
    sig = torch.from_numpy(synth.synth_tensor(0, "g3/sig", (96,), 0.8))[None].to(dev)
    sigt = torch.from_numpy(synth.synth_tensor(0, "g3/sigt", (42,), 0.8)).to(dev)
    H, W, n = sc["H"], sc["W"], a.rays
    bg_all = (torch.from_numpy(sc["bg"]).float() / 255.0).reshape(-1, 3).to(dev)
    pix32 = ((torch.arange(n, dtype=torch.int64) * 3163) % (H * W)).to(dev).to(torch.int32)
    tgt = torch.rand(n, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    buf = training.TrainBuffers(tier, n, dev, n_fine=n_fine)
    fr = engine.make_frame(H, W, sc["focal"], sc["cx"], sc["cy"], sc["poses"][0], sc["pose_body"], sc["near"], sc["far"], ray_count=n,
                           n_fine=n_fine, fields=2)
    decs, opts = {}, {}
    for key, kw in MODES:
        d = Decoder(z_dim=256, hidden_size=256, dim_signal=96, use_deformation_field=True)
        d.load_state_dict({k: torch.from_numpy(v) for k, v in st["decoder"].items()})
        decs[key] = d.to(dev)
        opts[key] = HipAdam(list(d.parameters()), lr=5e-4, betas=(0.9, 0.999), **kw)

    def step(key):
        opts[key].zero_grad()
        rh, rc = training.render_train(decs[key], buf, fr, bg_all, pix32, sig, sigt, zs[0, :2], za[0, :2])
        (((rh - tgt) ** 2).mean() + ((rc - tgt) ** 2).mean()).backward()
        opts[key].step()

    def timed(key):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            step(key)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps

    for key, _ in MODES:                                   # warm-up (code objects, clocks, the launch tables) + the results to compare
        for _ in range(3):
            step(key)
    torch.cuda.synchronize()
    same = all(torch.equal(p, q) for key in ("guard", "clip")
               for p, q in zip(decs["off"].parameters(), decs[key].parameters()))
    t = {key: [] for key, _ in MODES}
    for _ in range(a.rounds):
        for key, _ in MODES:
            t[key].append(timed(key))
    gs = opts["clip"].grad_stats()
    m = {k: statistics.median(v) for k, v in t.items()}
    spread = (max(t["off"]) - min(t["off"])) / m["off"]
    shape = "c4 (64)" if n_fine == 0 else f"c4h (64 + {n_fine})"
    rounds = lambda k: " ".join(f"{x:.3f}" for x in t[k])
    print(f"{shape:14s} {tier:5s} off: median {m['off']:7.3f} (rounds {rounds('off')}; spread {spread:.4f})  |  guard: median "
          f"{m['guard']:7.3f} (rounds {rounds('guard')})  |  clip: median {m['clip']:7.3f} (rounds {rounds('clip')})  |  guard / off = "
          f"{m['guard'] / m['off']:.4f}, clip / off = {m['clip'] / m['off']:.4f}  |  parameters bit-equal after warm-up: {same}; "
          f"skipped {gs['skipped_total']}, clip_coef {gs['clip_coef']}", flush=True)
    return 0 if same else 3


if a.child:
    tier, n_fine = a.child.split(":")
    sys.exit(child(tier, int(n_fine)))

lines = [f"grad_guard_ab: synthetic Decoder(hidden_size=256); {a.rays} rays, two fields, forward + backward (MSE on both images) + the "
         f"decoder's HipAdam step; off = unguarded, guard = skip_nonfinite, clip = skip_nonfinite + max_grad_norm 1e9 (never binds); "
         f"{a.rounds} interleaved rounds x {a.reps} steps per mode, device events; ms per step"]
print(lines[0], flush=True)
for tier in a.tiers.split(","):
    for n_fine in a.fine.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", f"{tier}:{int(n_fine)}", "--rays", str(a.rays), "--rounds",
               str(a.rounds), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"grad_guard_ab: {tier} / {n_fine} ran into its time limit ({a.limit} s): stopping here")
        rows = [ln for ln in r.stdout.splitlines() if ln.startswith("c4")]
        if r.returncode != 0 or not rows:
            sys.exit(f"grad_guard_ab: {tier} / {n_fine} failed (exit {r.returncode}): stopping here\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        print(rows[-1], flush=True)
        lines.append(rows[-1])
if a.out:
    with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
