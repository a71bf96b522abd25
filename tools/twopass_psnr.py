#!/usr/bin/env python3
"""Developer tool: does the f16 tier keep its accuracy clause on the blend decoder (tests/blend_scene.py) when an exact-class tier places
the fine samples?  The f16 accuracy guard's own sample (4 frames x 256 random pixels, seed 0, two fields, golden G7's conditioning) and
statistics (f16guard.accuracy_stats) at 32 + 32 and 64 + 128, every row against the f32 tier rendered at its own fine depths:

  plain f16            one launch: the f16 tier at its own fine depths (what the guard measures today)
  f16 @ f16x3 depths   engine.render_two_pass with the f16x3 tier as the sampler
  f16 @ f32 depths     engine.render_two_pass with the f32 tier as the sampler: the reference's own fine depths, bit for bit
  f16x3 one launch     for scale

  python tools/twopass_psnr.py [--out profiles/twopass_psnr.txt]"""
import argparse
import os
import sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
a = ap.parse_args()
lines = []
for p in ("dfa-nerf_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import blend_scene as B
from dfanerf import engine, f16guard, synth
dev = torch.device("cuda")
scene, states, latents = synth.bench_scene(0, n_frames=8), synth.synth_all_states(0), synth.synth_latents(0)
g7 = dict(np.load(os.path.join(ROOT, "tests", "golden", "g7_frame_coarse.npz")))
sa, stt, zs, za = B.conditioning(g7, latents)
flat = engine.flatten_state(B.blend_state(states), dev)
pk = {t: engine.PackedDecoder(flat, t) for t in ("f32", "f16", "f16x3")}
bias = {t: p.fold(sa, stt, zs, za) for t, p in pk.items()}
bg = (torch.from_numpy(scene["bg"]).float() / 255.0).reshape(-1, 3).to(dev)
gate = f16guard.psnr_gate(f16guard.DEFAULT_MODEL_PSNR)
for nc, nf in ((32, 32), (64, 128)):
    gen = torch.Generator(device="cpu").manual_seed(0)
    blocks = {"plain f16": [], "f16 @ f16x3 depths": [], "f16 @ f32 depths": [], "f16x3 one launch": []}
    for k in range(4):
        pix = torch.randperm(scene["H"] * scene["W"], generator=gen)[:256].to(torch.int32).to(dev)
        fr = engine.make_frame(scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"], scene["poses"][k], scene["pose_body"],
                               scene["near"], scene["far"], ray_count=256, n_coarse=nc, n_fine=nf, fields=2)
        ref = [x.clone() for x in engine.render(pk["f32"], bias["f32"], fr, bg, pix_index=pix)]
        img = {"plain f16": engine.render(pk["f16"], bias["f16"], fr, bg, pix_index=pix),
               "f16x3 one launch": engine.render(pk["f16x3"], bias["f16x3"], fr, bg, pix_index=pix)}
        img = {n: [x.clone() for x in v] for n, v in img.items()}
        for n, s in (("f16 @ f16x3 depths", "f16x3"), ("f16 @ f32 depths", "f32")):
            img[n] = [x.clone() for x in engine.render_two_pass(pk[s], bias[s], pk["f16"], bias["f16"], fr, bg, pix_index=pix)]
        for n, v in img.items():
            blocks[n].append({"head": (v[0], ref[0], None), "com": (v[1], ref[1], None)})
    for n, b in blocks.items():
        st = f16guard.accuracy_stats(b)
        lines.append(f"{nc}+{nf} {n:20s} " + "; ".join(f"{i} {st[i]['psnr_db']:.2f} dB (worst frame {st[i]['worst_block_db']:.2f}, max |err| {st[i]['max_abs']:.4f})"
                                                for i in ("head", "com")) + f"; gate {gate:.2f} dB (worst frame {gate - f16guard.BLOCK_SLACK_DB:.2f})")
        print(lines[-1], flush=True)
if a.out:
    with open(a.out if os.path.isabs(a.out) else os.path.join(ROOT, a.out), "w") as f:
        f.write("\n".join(lines) + "\n")
