"""The end-to-end pose fit of tests/test_gpu_ray_grad.py, shared between the library (on the GPU) and the oracle (torch CPU autograd):
256 pixels of one frame, targets = the images rendered at the true poses, start = a known translation offset on both origins plus a
small rotation of the head pose, 40 Adam steps on the 6 + 3 parameters through training.pinhole_rays.

    python tests/ray_grad_fit.py        the same fit through the oracle's autograd on the CPU: the numbers recorded in the test"""
import numpy as np
import torch

N_PIX, STEPS, LR = 256, 40, 1e-4
FRAME, NEAR, FAR = 1, 0.3, 0.9
# d t_head, d t_body, head rotation (rad).  Millimetre-scale: the synthetic field's top octaves make the loss non-convex beyond that (ten
# times these offsets: the oracle's own fit lowers the loss and not the pose error)
START = torch.tensor([0.0020, -0.0015, 0.0010, -0.0012, 0.0018, 0.0014, 0.0015, -0.0020, 0.0010])


def pixels(scene):
    return (torch.arange(N_PIX, dtype=torch.int64) * 3163 + 11) % (scene["H"] * scene["W"])


def _skew(w):
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])


def posed(scene, q, device="cpu"):
    """the two [3,4] poses of parameter vector q [9]: translations moved by q[0:3] / q[3:6], the head's rotation turned by exp([q[6:9]])"""
    P = torch.from_numpy(np.asarray(scene["poses"][FRAME], np.float32)[:3, :4].copy()).to(device)
    B = torch.from_numpy(np.asarray(scene["pose_body"], np.float32)[:3, :4].copy()).to(device)
    R = torch.matrix_exp(_skew(q[6:9])) @ P[:, :3]
    return torch.cat([R, (P[:, 3] + q[0:3])[:, None]], 1), torch.cat([B[:, :3], (B[:, 3] + q[3:6])[:, None]], 1)


def fit(scene, render, device="cpu"):
    """render(rays [n,12]) -> rgb_head, rgb_com.  Returns (losses [STEPS + 1], pose errors [STEPS + 1]): the value at the start of every
    step and after the last one; pose error = |q| (the truth is q = 0)."""
    from dfanerf import training
    geo = (scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"])
    pix = pixels(scene).to(device)
    with torch.no_grad():
        th, tc = render(training.pinhole_rays(*posed(scene, torch.zeros(9, device=device), device), pix, *geo))
        th, tc = th.detach().clone(), tc.detach().clone()
    q = START.clone().to(device).requires_grad_(True)
    opt = torch.optim.Adam([q], lr=LR)
    losses, errs = [], []
    for step in range(STEPS + 1):
        rh, rc = render(training.pinhole_rays(*posed(scene, q, device), pix, *geo))
        loss = ((rh - th) ** 2).mean() + ((rc - tc) ** 2).mean()
        losses.append(float(loss.detach()))
        errs.append(float(q.detach().norm()))
        if step == STEPS:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    return losses, errs


def oracle_render(scene, states, latents, sigs):
    import dfa_oracle as O
    P = O.params_to_torch(states["decoder"])
    zs, za = [torch.from_numpy(np.asarray(v)) for v in latents]
    bg = (torch.from_numpy(np.asarray(scene["bg"])).float() / 255.0).reshape(-1, 3)[pixels(scene)]
    z = O.coarse_z(NEAR, FAR, 64)[None].expand(N_PIX, 64)

    def render(rays):
        return O.render_fixed_samples(P, rays[:, 0:3], rays[:, 3:6], rays[:, 6:9], rays[:, 9:12], bg, z, zs, za, [sigs[0], None],
                                      sigs[1][None], 2)
    return render


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in ("dfa-nerf_amd", "oracle", "tests"):
        sys.path.insert(0, os.path.join(root, p))
    from dfanerf import synth
    from test_gpu_train_hier import _signals
    scene, states, latents = synth.bench_scene(0, n_frames=8), synth.synth_all_states(0), synth.synth_latents(0)
    losses, errs = fit(scene, oracle_render(scene, states, latents, _signals(states, scene)))
    print("oracle fit: loss %.6e -> %.6e, pose error %.6e -> %.6e" % (losses[0], losses[-1], errs[0], errs[-1]))
    print("losses", " ".join("%.3e" % v for v in losses))
    print("errors", " ".join("%.4e" % v for v in errs))
