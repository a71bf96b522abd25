#!/usr/bin/env python3
"""Developer tool, CPU only: the oracle half of tests/test_gpu_ray_grad.py::test_point_gradients_vs_oracle_autograd[torso-no_deform] -
autograd of the oracle's decoder_forward w.r.t. p_in and ray_d for the torso field of the decoder without the deformation field, in
float32 against float64, per point and with 1 thread as well as the default.  The f32 reference of that block depends on the host's CPU
(one ReLU at a tie at one of the 512 points: LABNOTES.md 15); this prints which way it falls here: the relative error of the f32 oracle
against float64, the four worst points, and the error without the worst one.

  python tools/diag_point_grad_reference.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("dfa-nerf_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
import dfa_oracle as O
from dfanerf import synth
from test_gpu_train_hier import _signals, t
from test_gpu_ray_grad import _points
print("threads", torch.get_num_threads(), "| torch", torch.__version__)
print([l for l in torch.__config__.show().split("\n") if "CPU capability" in l or "MKL" in l or "BLAS" in l][:6])
scene, states = synth.bench_scene(0, n_frames=8), synth.synth_all_states(0)
sigs = _signals(states, scene)
state = {k: v for k, v in synth.synth_decoder_state(0).items() if not k.startswith("deform_net.")}
zs, za = [t(v) for v in synth.synth_latents(0)]
p, d = _points()
g = torch.Generator().manual_seed(43)
w_f, w_s = torch.randn(1, p.shape[1], 3, generator=g), torch.randn(1, p.shape[1], generator=g)
for nthr in (None, 1):
    if nthr:
        torch.set_num_threads(nthr)
    ref = {}
    for dt in (torch.float32, torch.float64):
        P = {k: v.to(dt) for k, v in O.params_to_torch(state).items()}
        po, do = p.clone().to(dt).requires_grad_(True), d.clone().to(dt).requires_grad_(True)
        fo, sgo = O.decoder_forward(P, po, do, zs[:, 1].to(dt), za[:, 1].to(dt), sigs[1][None].to(dt), "torso")
        ((fo * w_f.to(dt)).sum() + (sgo * w_s.to(dt)).sum()).backward()
        ref[dt] = (po.grad.double()[0], do.grad.double()[0])
    for k, name in ((0, "d p_in"), (1, "d ray_d")):
        a, b = ref[torch.float32][k], ref[torch.float64][k]
        row = (a - b).norm(dim=-1)
        worst = torch.argsort(row, descending=True)[:4]
        print(f"threads {torch.get_num_threads()} {name}: f32 oracle vs float64 {float((a - b).norm() / b.norm()):.3e}; |ref| {float(b.norm()):.3e}; worst points "
              + ", ".join(f"#{int(i)} err {float(row[i]):.2e} (row norm {float(b[i].norm()):.2e})" for i in worst)
              + f"; without the worst point {float((a - b)[row < row.max()].norm() / b.norm()):.3e}")
