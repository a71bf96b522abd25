#!/usr/bin/env python3
"""Developer experiment (CPU, no GPU needed): accuracy of the f16x3 tier's split operands, emulated in torch.

Every decoder GEMM of the oracle (dfa_oracle._lin: weights AND activations) is replaced by the f16x3 product: x ~ hi + 2^-11 lo'
with hi = f16(x), lo' = f16((x - hi) 2^11), and hi.hi + 2^-11 (hi.lo' + lo'.hi) as an f32 matmul of f16-valued tensors (the
product of two f16 values is exact in f32, so this models v_mfma_f32_32x32x16_f16).  Conservative against the kernel: the per-frame
constants (signal columns, latent projections) are split too, where the kernel folds them into f32 biases.  Runs the oracle's row-H
pipeline (coarse -> sample_pdf -> merged pass -> compositing; golden G7's frame and rays, head and two fields, 64 + 128) and the
decoder on golden G3's points, with f16 subnormals kept and flushed (--flush both ways):
  PSNR of the split-operand image against the f32-operand image, the share of depths / rays identical to the golden's,
  max |dfeat| / |dsigma| against G3.
usage: python tools/emulate_split_tier.py [n_rays (<= 511)]"""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("dfa-nerf_amd", "oracle"):
    sys.path.insert(0, os.path.join(R, d))
import numpy as np, torch
import torch.nn.functional as F
import dfa_oracle as O
from dfanerf import synth

F16_MIN_NORMAL = 2.0 ** -14
_orig_lin = O._lin


def split(x, flush):
    hi = x.to(torch.float16).float()
    if flush:
        hi = torch.where(hi.abs() < F16_MIN_NORMAL, torch.zeros_like(hi), hi)
    lo = ((x - hi) * 2048.0).to(torch.float16).float()
    if flush:
        lo = torch.where(lo.abs() < F16_MIN_NORMAL, torch.zeros_like(lo), lo)
    return hi, lo


def make_lin(flush):
    def lin(P, name, x):
        W, b = P[name + ".weight"], P[name + ".bias"]
        xh, xl = split(x.float(), flush)
        wh, wl = split(W.float(), flush)
        return xh @ wh.T + (xh @ wl.T + xl @ wh.T) * (1.0 / 2048.0) + b
    return lin


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0 else -10.0 * np.log10(mse)


def main(n_rays):
    G = os.path.join(R, "tests", "golden")
    gh, gc, g3 = [dict(np.load(os.path.join(G, n + ".npz"))) for n in ("g7_frame_hier", "g7_frame_coarse", "g3_decoder")]
    sc = synth.bench_scene(0, n_frames=8)
    P = O.params_to_torch(synth.synth_all_states(0)["decoder"])
    zs, za = [torch.from_numpy(v) for v in synth.synth_latents(0)]
    idx = gh["ray_idx"][:n_rays]
    H, W = sc["H"], sc["W"]
    o_h, d_h = O.get_rays(H, W, sc["focal"], sc["poses"][2][:3, :4], sc["cx"], sc["cy"])
    o_t, d_t = O.get_rays(H, W, sc["focal"], sc["pose_body"][:3, :4], sc["cx"], sc["cy"])
    rays = [x.reshape(-1, 3)[idx] for x in (o_h, d_h, o_t, d_t)]
    bg = (torch.from_numpy(sc["bg"]).float() / 255.0).reshape(-1, 3)[idx]
    sig, sigt = [torch.from_numpy(gc["signal"]), None], torch.from_numpy(gc["signal_torso"])
    for fields in (1, 2):
        out = {}
        for mode in ("f32", "split", "split_flush"):
            O._lin = _orig_lin if mode == "f32" else make_lin(mode == "split_flush")
            with torch.no_grad():
                rh, rc, aux = O.render_rays_chunk(P, *rays, bg, sc["near"], sc["far"], zs, za, sig, sigt, 64, 128, fields,
                                                  return_aux=True)
            out[mode] = (rc if fields == 2 else rh, aux["z_all"])
        O._lin = _orig_lin
        zref = torch.from_numpy(gh[f"z_all_f{fields}"][:n_rays])
        for mode in ("f32", "split", "split_flush"):
            img, z = out[mode]
            dz = (z - zref).abs()
            line = f"fields={fields} {mode:11s}: depths identical to G7-hier (2e-6) {float((dz <= 2e-6).double().mean()) * 100:.3f} %, " \
                   f"rays {float((dz <= 2e-6).all(1).double().mean()) * 100:.1f} %"
            if mode != "f32":
                line += f"; image vs f32 operands {psnr(img, out['f32'][0]):.1f} dB, max |dRGB| {float((img - out['f32'][0]).abs().max()):.2e}"
            print(line, flush=True)
    for mode in ("split", "split_flush"):
        O._lin = make_lin(mode == "split_flush")
        worst_f = worst_s = 0.0
        for field, name in ((0, "head"), (1, "torso")):
            s = torch.from_numpy(g3["sig_aud"]) if field == 0 else torch.from_numpy(g3["sig_torso"])
            with torch.no_grad():
                f, sg = O.decoder_forward(P, torch.from_numpy(g3["p_192"]), torch.from_numpy(g3["r_192"]), zs[:, field], za[:, field],
                                          [s, None] if field == 0 else s, name)
            worst_f = max(worst_f, float((f - torch.from_numpy(g3[f"feat_{name}_192"])).abs().max()))
            worst_s = max(worst_s, float((sg - torch.from_numpy(g3[f"sigma_{name}_192"])).abs().max()))
        O._lin = _orig_lin
        print(f"G3 decoder, {mode}: max |dfeat| {worst_f:.2e}, max |dsigma| {worst_s:.2e}")


if __name__ == "__main__":
    torch.set_num_threads(min(8, torch.get_num_threads()))
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 128)
