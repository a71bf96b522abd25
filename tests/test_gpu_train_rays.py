"""GPU tests of the fused training step on CALLER-SUPPLIED rays: dfn_train_rays_fwd / dfn_train_rays_fwd_hier (the training forwards
render_kernel<TIER | TIER_RAYS, true, TRAIN>: csrc/dfn_render_variant.hip built as dfn_render_*_rays_train) and
dfn_composite_bwd_rays_z / dfn_composite_bwd_hier_rays_z (the RAYS instantiations of composite_bwd_kernel, coarse and hierarchical), through
training.render_train(rays=, bounds=).

  1. pinhole rays supplied = the plain step, bit for bit: images, raw samples, recorded activations and ReLU masks, every decoder
     gradient and both signal gradients (f32, bf16 with both recorder formats; coarse and hierarchical; with and without bounds);
  2. the two compositing backward kernels on their own against torch autograd through the oracle's integrate_fields;
  3. the whole step on rays no pinhole makes (sub-pixel offsets, rescaled directions, per-ray bounds) against the oracle under autograd
     at the kernel's own depths, at the gates of tests/test_gpu_train_hier.py;
  4. ten Adam steps lower the loss; one step twice gives the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import dfa_oracle as O
from test_gpu_train_hier import _decoder, _signals, t

pytestmark = pytest.mark.gpu

NEAR, FAR = 0.3, 0.9
FRAME = 1


@pytest.fixture(scope="module")
def sigs(states, scene):
    return _signals(states, scene)


def _pixels(scene, n, seed=0):
    return (torch.arange(n, dtype=torch.int64) * 3163 + 17 * seed) % (scene["H"] * scene["W"])


def _plain_frame(scene, n, n_coarse, n_fine):
    from dfanerf import engine
    return engine.make_frame(scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"], scene["poses"][FRAME], scene["pose_body"],
                             NEAR, FAR, 1e10, 0, n, n_coarse, n_fine, 2, True)


def _rays_frame(n, n_coarse, n_fine, near=NEAR, far=FAR):
    """the frame of a rays launch: sample counts and near / far; poses, intrinsics, H, W are ignored - filled with junk on purpose"""
    from dfanerf import engine
    junk = np.full((4, 4), 7.5, np.float32)
    return engine.make_frame(3, 5, 1.0, -2.0, 9.0, junk, junk, near, far, 1e10, 11, n, n_coarse, n_fine, 2, True)


def _step(states, scene, latents, sigs, tier, fmt, n_coarse, n_fine, n, frame, bg, pix=None, rays=None, bounds=None, tgt_seed=5):
    """one forward + backward through training.render_train -> everything the step leaves behind, on the CPU"""
    from dfanerf import training
    dev = torch.device("cuda")
    zs, za = [t(v).to(dev) for v in latents]
    tgt = torch.rand(n, 3, generator=torch.Generator().manual_seed(tgt_seed))
    dec = _decoder(states, dev)
    sh = sigs[0].to(dev).requires_grad_(True)
    st = sigs[1].to(dev).requires_grad_(True)
    buf = training.TrainBuffers(tier, n, dev, n_fine=n_fine, act_format=fmt, n_coarse=n_coarse)
    for a in buf.act + buf.masks:        # (the recorder leaves structural padding untouched: compare like with like)
        a.zero_()
    rh, rc = training.render_train(dec, buf, frame, bg, None if pix is None else pix.to(dev, torch.int32), sh, st, zs[0, :2],
                                   za[0, :2], rays=rays, bounds=bounds)
    loss = ((rh - tgt.to(dev)) ** 2).mean() + ((rc - tgt.to(dev)) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.detach().cpu().clone()) for k, p in dec.named_parameters()}
    out = dict(rh=rh.detach().cpu(), rc=rc.detach().cpu(), loss=loss.item(), d_sh=sh.grad.cpu(), d_st=st.grad.cpu(), grads=grads,
               tgt=tgt, samples=buf.samples.cpu(), dsamples=buf.dsamples.cpu(), act=[a.cpu() for a in buf.act],
               masks=[m.cpu() for m in buf.masks])
    if n_fine:
        out.update(z=buf.z_all.cpu(), ranks=buf.ranks.cpu())
    return out


def _pinhole_rays(scene, pix):
    """engine.pack_rays of dfn_get_rays for the frame's two poses, gathered at the pixels"""
    from dfanerf import engine
    geo = (scene["H"], scene["W"], scene["focal"])
    o_h, d_h = engine.get_rays(*geo, scene["poses"][FRAME], scene["cx"], scene["cy"])
    o_t, d_t = engine.get_rays(*geo, scene["pose_body"], scene["cx"], scene["cy"])
    sel = pix.cuda()
    return engine.pack_rays(*(x.reshape(-1, 3)[sel] for x in (o_h, d_h, o_t, d_t)))


def _assert_same_step(a, b, what, hier):
    keys = ["rh", "rc", "samples", "dsamples", "d_sh", "d_st"] + (["z", "ranks"] if hier else [])
    for k in keys:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].float() - b[k].float()).abs().max()))
    for k in ("act", "masks"):
        for f in (0, 1):
            assert torch.equal(a[k][f], b[k][f]), (what, k, f)
    assert a["loss"] == b["loss"], what
    n_grads = 0
    for k, g in a["grads"].items():
        h = b["grads"][k]
        assert (g is None) == (h is None), (what, k)
        if g is not None:
            assert torch.equal(g, h), (what, k, float((g - h).abs().max()))
            n_grads += 1
    assert n_grads > 40, n_grads


def _identity_case(states, scene, latents, sigs, tier, fmt, n_coarse, n_fine, n):
    dev = torch.device("cuda")
    pix = _pixels(scene, n)
    bg_all = (t(scene["bg"]).float() / 255.0).reshape(-1, 3).to(dev)
    plain = _step(states, scene, latents, sigs, tier, fmt, n_coarse, n_fine, n, _plain_frame(scene, n, n_coarse, n_fine), bg_all, pix=pix)
    assert float(plain["rh"].std()) > 0 and sum(float(g.abs().max()) > 0 for g in plain["grads"].values() if g is not None) > 40
    rays = _pinhole_rays(scene, pix)
    bg = bg_all[pix.to(dev)].contiguous()
    fr = _rays_frame(n, n_coarse, n_fine)
    got = _step(states, scene, latents, sigs, tier, fmt, n_coarse, n_fine, n, fr, bg, rays=rays)
    _assert_same_step(plain, got, "no bounds", n_fine > 0)
    # per-ray bounds filled with the frame's pair; the frame's own pair is junk then
    bounds = torch.tensor([NEAR, FAR], dtype=torch.float32, device=dev).repeat(n, 1)
    fr = _rays_frame(n, n_coarse, n_fine, near=5.0, far=6.0)
    got = _step(states, scene, latents, sigs, tier, fmt, n_coarse, n_fine, n, fr, bg, rays=rays, bounds=bounds)
    _assert_same_step(plain, got, "bounds", n_fine > 0)


@pytest.mark.parametrize("tier,fmt", [("f32", None), ("bf16", "fp4"), ("bf16", "e4m3")])
def test_pinhole_rays_equal_the_plain_step_bit_for_bit_coarse(states, scene, latents, sigs, tier, fmt):
    """48 rays at 32 coarse samples: NP = 1536 is an odd number of 512-point blocks - six workgroups in the bf16 tier, twelve in f32"""
    _identity_case(states, scene, latents, sigs, tier, fmt, 32, 0, 48)


@pytest.mark.parametrize("tier,fmt", [("f32", None), ("bf16", "fp4")])
def test_pinhole_rays_equal_the_plain_step_bit_for_bit_hier(states, scene, latents, sigs, tier, fmt):
    """16 rays at 64 + 64: z_all and ranks too"""
    _identity_case(states, scene, latents, sigs, tier, fmt, 64, 64, 16)


# ---- the compositing backward on its own ---------------------------------------------------------------------------------------------
def _random_rays(rs, n):
    """origins near the scene's, directions of length 0.5 ... 2 (head and torso independently)"""
    o = rs.uniform(-0.1, 0.1, size=(n, 2, 3)).astype(np.float32)
    d = rs.randn(n, 2, 3).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d *= rs.uniform(0.5, 2.0, size=(n, 2, 1)).astype(np.float32)
    return np.concatenate([o[:, 0], d[:, 0], o[:, 1], d[:, 1]], 1).astype(np.float32)


def _random_samples(rs, n, S):
    samples = rs.randn(n, S, 8).astype(np.float32)
    samples[..., 0] = samples[..., 0] * 8 - 2
    samples[..., 4] = samples[..., 4] * 8 - 2
    samples[..., 1:4] = 1 / (1 + np.exp(-samples[..., 1:4]))
    samples[..., 5:8] = 1 / (1 + np.exp(-samples[..., 5:8]))
    samples[3, S // 6:S // 2, 0] = -1.0
    samples[3, S // 6:S // 2, 4] = -1.0                                  # both fields empty -> the 1e-4 denominator branch
    return samples


def _per_ray_coarse_z(bounds, n_coarse):
    """MAIN:617-618 with each ray's own pair: near * (1 - t) + far * t, f32"""
    tt = O.linspace01(n_coarse)
    return bounds[:, :1] * (1.0 - tt)[None] + bounds[:, 1:] * tt[None]


@pytest.mark.parametrize("n_coarse,n_fine", [(32, 0), (128, 0), (64, 64), (64, 128)])
def test_composite_backward_rays_vs_autograd(n_coarse, n_fine):
    """dfn_composite_bwd_rays_z / dfn_composite_bwd_hier_rays_z on 5 rays (the second workgroup holds one live wave): random raw
    samples, directions scaled by 0.5 ... 2, per-ray bounds (coarse) / random sorted depths and a random rank permutation
    (hierarchical), against torch autograd through the oracle's integrate_fields - as test_composite_backward_hier_vs_autograd does,
    at its tolerance.  The zero-fill buffer is filled; dsamples holds nothing of its poison."""
    from dfanerf._lib import check, lib
    n, S = 5, n_coarse + n_fine
    rs = np.random.RandomState(11 + S)
    samples = _random_samples(rs, n, S)
    rays = _random_rays(rs, n)
    bounds = np.stack([0.3 + rs.uniform(0, 0.05, n), 0.9 - rs.uniform(0, 0.05, n)], 1).astype(np.float32)
    bg = rs.uniform(0, 1, size=(n, 3)).astype(np.float32)
    d_h, d_c = rs.randn(n, 3).astype(np.float32), rs.randn(n, 3).astype(np.float32)
    dev = "cuda"
    fr = _rays_frame(n, n_coarse, n_fine, near=5.0, far=6.0)            # (coarse: the bounds replace the frame's pair)
    ds = torch.full((n, S, 8), float("nan"), device=dev)
    zero = torch.full((1031,), 7.0, device=dev)                           # (not a multiple of four floats: the fill's tail too)
    Sd, RY, BD, BG, DH, DC = [t(a).to(dev).contiguous() for a in (samples, rays, bounds, bg, d_h, d_c)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sm = t(samples).clone().requires_grad_(True)
    if n_fine:
        z = np.sort(rs.uniform(0.3, 0.9, size=(n, S)).astype(np.float32), axis=1)
        ranks = np.stack([rs.permutation(S) for _ in range(n)]).astype(np.uint8)      # ranks[r, e] = merged position of point e
        Z, RK = t(z).to(dev).contiguous(), t(ranks).to(dev).contiguous()
        check(lib.dfn_composite_bwd_hier_rays_z(C.byref(fr), RY.data_ptr(), BD.data_ptr(), BG.data_ptr(), None, Sd.data_ptr(),
                                                Z.data_ptr(), RK.data_ptr(), DH.data_ptr(), DC.data_ptr(), ds.data_ptr(),
                                                zero.data_ptr(), zero.numel(), st), "dfn_composite_bwd_hier_rays_z")
        idx = t(ranks.astype(np.int64))
        inv = torch.empty_like(idx)
        inv.scatter_(1, idx, torch.arange(S)[None].expand(n, S))          # inv[r, m] = evaluation index at merged position m
        merged = torch.gather(sm, 1, inv[..., None].expand(n, S, 8))
        zt = t(z)
    else:
        check(lib.dfn_composite_bwd_rays_z(C.byref(fr), RY.data_ptr(), BD.data_ptr(), BG.data_ptr(), None, Sd.data_ptr(),
                                           DH.data_ptr(), DC.data_ptr(), ds.data_ptr(), zero.data_ptr(), zero.numel(), st),
              "dfn_composite_bwd_rays_z")
        merged = sm
        zt = _per_ray_coarse_z(t(bounds), n_coarse)
    torch.cuda.synchronize()
    rh, _, rc, _ = O.integrate_fields(zt, t(rays[:, 3:6]), t(rays[:, 9:12]), merged[..., 0], merged[..., 1:4], merged[..., 4],
                                      merged[..., 5:8], t(bg))
    ((rh * t(d_h)).sum() + (rc * t(d_c)).sum()).backward()
    got, ref = ds.cpu().numpy(), sm.grad.numpy()
    assert float(zero.abs().max()) == 0.0
    assert np.isfinite(got).all()
    assert np.abs(ref).max() > 0
    np.testing.assert_allclose(got, ref, atol=2e-5 * np.abs(ref).max(), rtol=2e-4)


# ---- the whole step on rays no pinhole makes -------------------------------------------------------------------------------------------
def _jittered_rays(scene, pix, seed):
    """each pixel's two rays (HELP:449-465) moved by a uniform sub-pixel offset, directions rescaled per ray by 0.5 ... 2 (head and torso
    independently), and bounds (0.3 + U(0, 0.05), 0.9 - U(0, 0.05)) -> o_h, d_h, o_t, d_t [n,3], bounds [n,2] (CPU, f32)"""
    g = torch.Generator().manual_seed(seed)
    n = pix.numel()
    W = scene["W"]
    y, x = (pix // W).float(), (pix % W).float()
    off = torch.rand(n, 2, generator=g) - 0.5
    dirs = torch.stack([(x + off[:, 0] - scene["cx"]) / scene["focal"], -(y + off[:, 1] - scene["cy"]) / scene["focal"],
                        -torch.ones(n)], -1)
    out = []
    for pose in (scene["poses"][FRAME], scene["pose_body"]):
        c2w = t(np.asarray(pose, np.float32)[:3, :4])
        d = dirs @ c2w[:, :3].T
        d = d * (0.5 + 1.5 * torch.rand(n, 1, generator=g))
        out += [c2w[:, 3][None].expand(n, 3).contiguous(), d.contiguous()]
    bounds = torch.stack([0.3 + 0.05 * torch.rand(n, generator=g), 0.9 - 0.05 * torch.rand(n, generator=g)], 1)
    return out, bounds.float().contiguous()


@pytest.mark.parametrize("tier,n_fine", [("f32", 0), ("f32", 128), ("bf16", 0), ("bf16", 128)])
def test_jittered_rays_step_vs_oracle_autograd(states, scene, latents, sigs, tier, n_fine):
    """Loss, images and EVERY gradient of the step on 64 jittered, rescaled rays with per-ray bounds against torch CPU autograd
    through the oracle's render_fixed_samples at the kernel's own depths (coarse: near * (1 - t) + far * t per ray; hierarchical:
    z_all, sorted, ending at that ray's far), at the gates of test_hierarchical_training_step_vs_oracle_autograd."""
    from dfanerf import engine
    dev = torch.device("cuda")
    n, S = 64, 64 + n_fine
    pix = _pixels(scene, n)
    r4, bounds = _jittered_rays(scene, pix, seed=7)
    bg = (t(scene["bg"]).float() / 255.0).reshape(-1, 3)[pix].contiguous()
    rays = engine.pack_rays(*[x.to(dev) for x in r4])
    fr = _rays_frame(n, 64, n_fine, near=5.0, far=6.0)
    r = _step(states, scene, latents, sigs, tier, None, 64, n_fine, n, fr, bg.to(dev), rays=rays, bounds=bounds.to(dev))
    if n_fine:
        z = r["z"]
        assert bool((z[:, 1:] >= z[:, :-1]).all()) and torch.equal(z[:, -1], bounds[:, 1]) and torch.equal(z[:, 0], bounds[:, 0])
        ranks = r["ranks"].long()
        assert bool((torch.sort(ranks, 1).values == torch.arange(S)[None]).all())
        assert torch.equal(torch.gather(z, 1, ranks[:, :64]), _per_ray_coarse_z(bounds, 64))
    else:
        z = _per_ray_coarse_z(bounds, 64)
    P = O.params_to_torch(states["decoder"])
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    sh_o = sigs[0].clone().requires_grad_(True)
    st_o = sigs[1].clone()[None].requires_grad_(True)
    zs, za = [t(v) for v in latents]
    oh, oc = O.render_fixed_samples(Pg, *r4, bg, z, zs, za, [sh_o, None], st_o, 2)
    lo = ((oh - r["tgt"]) ** 2).mean() + ((oc - r["tgt"]) ** 2).mean()
    lo.backward()
    rel_err = lambda a, b: float((a.reshape(-1) - b.reshape(-1)).norm() / (b.norm() + 1e-30))
    e_img = max(float((r["rh"] - oh.detach()).abs().max()), float((r["rc"] - oc.detach()).abs().max()))
    e_loss = abs(r["loss"] - lo.item()) / abs(lo.item())
    e_sig = max(rel_err(r["d_sh"], sh_o.grad), rel_err(r["d_st"], st_o.grad))
    f32 = tier == "f32"
    rel = 1e-3 if f32 else 6e-2
    worst_n = worst_t = 0.0
    bad = []
    for k, g in r["grads"].items():
        ref = Pg[k].grad
        if k.startswith(("fc_in_listener", "fc_p_skips_listener")):
            assert g is None and (ref is None or float(ref.abs().max()) == 0.0), k
            continue
        rn = float(ref.double().norm())
        assert g is not None, k
        if rn == 0.0:
            assert float(g.abs().max()) <= 1e-12, k
            continue
        gn, e = float(g.double().norm()), rel_err(g, ref)           # the norm, and the whole-tensor direction
        worst_n, worst_t = max(worst_n, abs(gn - rn) / rn), max(worst_t, e)
        if not (abs(gn - rn) <= rel * rn + 1e-9 and e < (2e-3 if f32 else 1.5e-1)):
            bad.append((k, gn, rn, e))
    print(f"rays step {tier} n_fine={n_fine}: images {e_img:.2e}, loss {e_loss:.2e}, signals {e_sig:.2e}, worst gradient norm "
          f"{worst_n:.2e}, worst whole tensor {worst_t:.2e}")
    assert e_img < (5e-5 if f32 else 3e-2)
    assert e_loss <= (3e-5 if f32 else 2e-2)
    assert e_sig < 2 * rel
    assert not bad, bad


def test_jittered_rays_step_trains_and_is_bit_reproducible(states, scene, latents, sigs):
    """bf16 tier, 64 jittered rays with per-ray bounds: two runs of one step give identical losses and gradients (fixed-order
    reductions), and ten Adam steps on the fixed batch lower the loss."""
    from dfanerf import engine, run_nerf, training
    dev = torch.device("cuda")
    n = 64
    pix = _pixels(scene, n)
    r4, bounds = _jittered_rays(scene, pix, seed=9)
    bg = (t(scene["bg"]).float() / 255.0).reshape(-1, 3)[pix].contiguous().to(dev)
    rays, bounds = engine.pack_rays(*[x.to(dev) for x in r4]), bounds.to(dev)
    fr = _rays_frame(n, 64, 0)
    a = _step(states, scene, latents, sigs, "bf16", None, 64, 0, n, fr, bg, rays=rays, bounds=bounds)
    b = _step(states, scene, latents, sigs, "bf16", None, 64, 0, n, fr, bg, rays=rays, bounds=bounds)
    _assert_same_step(a, b, "two runs", False)
    zs, za = [t(v).to(dev) for v in latents]
    tgt = torch.rand(n, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    dec = _decoder(states, dev)
    opt = run_nerf.make_adam(dec.parameters(), 5e-4)
    buf = training.TrainBuffers("bf16", n, dev)
    sh, st = [x.to(dev) for x in sigs]
    losses = []
    for _ in range(10):
        rh, rc = training.render_train(dec, buf, fr, bg, None, sh, st, zs[0, :2], za[0, :2], rays=rays, bounds=bounds)
        loss = ((rh - tgt) ** 2).mean() + ((rc - tgt) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
