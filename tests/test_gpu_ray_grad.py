"""GPU tests of the ray gradients of the fused training step (f32 tier): dfn_composite_bwd_rays_zg / _hier_rays_zg (the <.., RAYS, DN>
compositing backward kernels: + the gradient of the ray norms), dfn_points_grad (points_grad_kernel), dfn_rays_grad (rays_grad_kernel),
through training.render_train with rays that require grad, Decoder.forward with points that do, and training.pinhole_rays.

  (a) d_norm of both _zg kernels against torch autograd through the oracle's integrate_fields; dsamples bit-equal to the _rays_z launch;
  (b) dfn_points_grad alone (through DecoderTrainFn) against autograd of the oracle's decoder_forward w.r.t. p_in and ray_d;
  (c) the whole step on 64 jittered, rescaled rays with per-ray bounds: rays.grad against the oracle's autograd, everything else
      bit-equal to the step whose rays do not require grad;
  (d) two runs give identical bits;
  (e) an end-to-end pose fit through pinhole_rays against the same fit through the oracle.

Gate of (b) and (c): the one tests/test_gpu_train_rays.py applies to d(signal) in the f32 tier - the other input gradient of the same
step: |got - ref| / |ref| < 2e-3 (Euclidean norms), per block and for the whole tensor."""
import ctypes as C

import numpy as np
import pytest
import torch

import dfa_oracle as O
import ray_grad_fit as FIT
from test_gpu_train_hier import _decoder, _signals, t
from test_gpu_train_rays import (_assert_same_step, _jittered_rays, _per_ray_coarse_z, _pixels, _random_rays, _random_samples,
                                 _rays_frame, _step)

pytestmark = pytest.mark.gpu

GATE = 2e-3          # test_jittered_rays_step_vs_oracle_autograd: e_sig < 2 * rel, rel = 1e-3 in the f32 tier


@pytest.fixture(scope="module")
def sigs(states, scene):
    return _signals(states, scene)


def rel_err(a, b):
    a, b = a.detach().double().reshape(-1).cpu(), b.detach().double().reshape(-1).cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


# ---- (a) the norm gradients of the compositing backward --------------------------------------------------------------------------------
@pytest.mark.parametrize("last_dist", [1e10, 0.05])
@pytest.mark.parametrize("concate_bg", [True, False])
@pytest.mark.parametrize("n_coarse,n_fine", [(32, 0), (64, 0), (128, 0), (64, 64), (64, 128)])
def test_norm_gradient_vs_autograd(n_coarse, n_fine, concate_bg, last_dist):
    """96 rays (24 workgroups of four waves; with 32 samples half of every wave idles): d_norm against torch autograd through the
    oracle's integrate_fields with the two ray norms as leaves (d = unit vector x norm) - the restatement and the tolerance of
    test_composite_backward_rays_vs_autograd - and dsamples bit for bit the _rays_z launch's."""
    from dfanerf import engine
    from dfanerf._lib import check, lib
    n, S = 96, n_coarse + n_fine
    rs = np.random.RandomState(23 + S)
    samples = _random_samples(rs, n, S)
    rays = _random_rays(rs, n)
    bounds = np.stack([0.3 + rs.uniform(0, 0.05, n), 0.9 - rs.uniform(0, 0.05, n)], 1).astype(np.float32)
    bg = rs.uniform(0, 1, size=(n, 3)).astype(np.float32)
    d_h, d_c = rs.randn(n, 3).astype(np.float32), rs.randn(n, 3).astype(np.float32)
    dev = "cuda"
    junk = np.full((4, 4), 7.5, np.float32)
    fr = engine.make_frame(3, 5, 1.0, -2.0, 9.0, junk, junk, 5.0, 6.0, last_dist, 11, n, n_coarse, n_fine, 2, concate_bg)
    Sd, RY, BD, BG, DH, DC = [t(a).to(dev).contiguous() for a in (samples, rays, bounds, bg, d_h, d_c)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ds = [torch.full((n, S, 8), float("nan"), device=dev) for _ in (0, 1)]
    dn = torch.full((n, 2), float("nan"), device=dev)
    sm = t(samples).clone()
    if n_fine:
        z = np.sort(rs.uniform(0.3, 0.9, size=(n, S)).astype(np.float32), axis=1)
        ranks = np.stack([rs.permutation(S) for _ in range(n)]).astype(np.uint8)
        Z, RK = t(z).to(dev).contiguous(), t(ranks).to(dev).contiguous()
        head = (C.byref(fr), RY.data_ptr(), BD.data_ptr(), BG.data_ptr(), None, Sd.data_ptr(), Z.data_ptr(), RK.data_ptr(), DH.data_ptr(),
                DC.data_ptr())
        check(lib.dfn_composite_bwd_hier_rays_z(*head, ds[0].data_ptr(), None, 0, st), "dfn_composite_bwd_hier_rays_z")
        check(lib.dfn_composite_bwd_hier_rays_zg(*head, ds[1].data_ptr(), None, 0, dn.data_ptr(), st), "dfn_composite_bwd_hier_rays_zg")
        idx = t(ranks.astype(np.int64))
        inv = torch.empty_like(idx)
        inv.scatter_(1, idx, torch.arange(S)[None].expand(n, S))
        merged = torch.gather(sm, 1, inv[..., None].expand(n, S, 8))
        zt = t(z)
    else:
        head = (C.byref(fr), RY.data_ptr(), BD.data_ptr(), BG.data_ptr(), None, Sd.data_ptr(), DH.data_ptr(), DC.data_ptr())
        check(lib.dfn_composite_bwd_rays_z(*head, ds[0].data_ptr(), None, 0, st), "dfn_composite_bwd_rays_z")
        check(lib.dfn_composite_bwd_rays_zg(*head, ds[1].data_ptr(), None, 0, dn.data_ptr(), st), "dfn_composite_bwd_rays_zg")
        merged = sm
        zt = _per_ray_coarse_z(t(bounds), n_coarse)
    torch.cuda.synchronize()
    assert torch.equal(ds[0], ds[1]) and bool(torch.isfinite(ds[1]).all())
    dirs = [t(rays[:, 3:6]), t(rays[:, 9:12])]
    norms = [d.norm(dim=-1).clone().requires_grad_(True) for d in dirs]
    unit = [d / d.norm(dim=-1, keepdim=True) for d in dirs]
    rh, _, rc, _ = O.integrate_fields(zt, unit[0] * norms[0][:, None], unit[1] * norms[1][:, None], merged[..., 0], merged[..., 1:4],
                                      merged[..., 4], merged[..., 5:8], t(bg), last_dist, concate_bg)
    ((rh * t(d_h)).sum() + (rc * t(d_c)).sum()).backward()
    got, ref = dn.cpu().numpy(), torch.stack([norms[0].grad, norms[1].grad], 1).numpy()
    print(f"d_norm {n_coarse}+{n_fine} bg={concate_bg} last={last_dist:g}: max|ref| {np.abs(ref).max():.3e}, max|got - ref| "
          f"{np.abs(got - ref).max():.3e}")
    assert np.isfinite(got).all() and np.abs(ref).max() > 0
    np.testing.assert_allclose(got, ref, atol=2e-5 * np.abs(ref).max(), rtol=2e-4)


# ---- (b) dfn_points_grad alone ---------------------------------------------------------------------------------------------------------
def _points(n=512):
    """512 points (sixteen tiles: two workgroups of eight waves) around the scene's volume, 64 of them at large coordinates (arguments
    of the top octave beyond 10^3), directions of length 0.5 ... 2"""
    g = torch.Generator().manual_seed(41)
    p = 0.3 * torch.randn(1, n, 3, generator=g)
    p[0, ::8] *= 8.0
    d = torch.randn(1, n, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True) * (0.5 + 1.5 * torch.rand(1, n, 1, generator=g))
    return p, d


DECODERS = {"scripts": dict(z_dim=256, hidden=256, deform=True), "narrow": dict(z_dim=64, hidden=128, deform=True),
            "no_deform": dict(z_dim=256, hidden=256, deform=False)}


# blocks of d ray_d whose f32 REFERENCE is, on some hosts, off by more than the gate against float64 (a ReLU tie: see the test's docstring):
# where such a block misses the ordinary gate it is gated at 4 x that error, against float64
F64_YARDSTICK_BLOCKS = {("no_deform", "torso")}


@pytest.mark.parametrize("which", sorted(DECODERS))
@pytest.mark.parametrize("field", ["head", "torso", "listener"])
def test_point_gradients_vs_oracle_autograd(sigs, which, field):
    """Decoder.forward at 512 explicit points with p_in and ray_d requiring grad: dfn_points_grad behind the dX chain (+ the
    normalisation's Jacobian for ray_d) against autograd of the oracle's decoder_forward, for the scripts' decoder, a narrower one
    (G18's shape: hidden 128, z 64 - the padded layout) and one without the deformation field (an all-zero net in the padded layout).
    Measured (MI355X), relative error against the f32 oracle: d p_in 5.2e-07 ... 5.3e-05, d ray_d 3.6e-07 ... 7.6e-07 - except, on some
    hosts, ONE block: d ray_d of the torso field without the deformation field.  The f32 reference there depends on the CPU that
    computes it: at point #278 of the 512 the f32 oracle jumps away from the float64 oracle under one CPU's GEMM kernels and not under another's -
    the signature of one ReLU at a tie deciding the other way (the unit was not located) (same torch build; 1 or 16 threads make no difference).  Where it
    decides the same (the build machine), the f32 oracle is 1.74e-06 from float64 and the library meets the ordinary gate.  Where it
    does not (the MI355X hosts this was measured on), the f32 oracle is 7.58e-03 from float64 - 1.05e-01 of error in that one row,
    1.74e-06 without it - while the library is 1.74e-06 from float64, so it reads 7.58e-03 against the f32 oracle: over the gate
    through the reference's flip, not its own.  For that block only, and only when it misses the ordinary gate, the rule the issue
    lays down applies: library against float64 <= 4 x the f32 oracle's own error against float64, both measured in this run.  Every
    other block keeps the d(signal) gate against the f32 oracle."""
    from dfanerf import synth
    from dfanerf.decoder import Decoder
    cfg = DECODERS[which]
    dev = torch.device("cuda")
    state = synth.synth_decoder_state(0, z_dim=cfg["z_dim"], hidden=cfg["hidden"])
    if not cfg["deform"]:
        state = {k: v for k, v in state.items() if not k.startswith("deform_net.")}
    dec = Decoder(z_dim=cfg["z_dim"], hidden_size=cfg["hidden"], dim_signal=96, use_deformation_field=cfg["deform"])
    dec.load_state_dict({k: t(v) for k, v in state.items()})
    dec.to(dev)
    zs, za = [t(v) for v in synth.synth_latents(0, z_dim=cfg["z_dim"])]
    row = 1 if field == "torso" else 0
    p, d = _points()
    g = torch.Generator().manual_seed(43)
    w_f, w_s = torch.randn(1, p.shape[1], 3, generator=g), torch.randn(1, p.shape[1], generator=g)
    sig = {"head": [sigs[0], None], "torso": sigs[1][None], "listener": [None, None]}[field]
    sig_dev = {"head": [sigs[0].to(dev), None], "torso": sigs[1].to(dev), "listener": [None, None]}[field]
    pg, dg = p.clone().to(dev).requires_grad_(True), d.clone().to(dev).requires_grad_(True)
    feat, sigma = dec(pg, dg, zs[:, row].to(dev), za[:, row].to(dev), sig_dev, "torso" if field == "torso" else "head")
    ((feat * w_f.to(dev)).sum() + (sigma * w_s.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    ref = {}
    for dt in (torch.float32, torch.float64):
        P = {k: v.to(dt) for k, v in O.params_to_torch(state).items()}
        po, do = p.clone().to(dt).requires_grad_(True), d.clone().to(dt).requires_grad_(True)
        cast = lambda s: None if s is None else s.to(dt)
        so = [cast(s) for s in sig] if isinstance(sig, list) else cast(sig)
        fo, sgo = O.decoder_forward(P, po, do, zs[:, row].to(dt), za[:, row].to(dt), so, "torso" if field == "torso" else "head")
        ((fo * w_f.to(dt)).sum() + (sgo * w_s.to(dt)).sum()).backward()
        ref[dt] = (po.grad, do.grad)
    e_p, e_d = rel_err(pg.grad, ref[torch.float32][0]), rel_err(dg.grad, ref[torch.float32][1])
    y_p, y_d = rel_err(ref[torch.float32][0], ref[torch.float64][0]), rel_err(ref[torch.float32][1], ref[torch.float64][1])
    print(f"points {which} {field}: d p_in {e_p:.2e} vs the f32 oracle ({rel_err(pg.grad, ref[torch.float64][0]):.2e} vs float64; the f32 "
          f"oracle's own {y_p:.2e}), d ray_d {e_d:.2e} ({rel_err(dg.grad, ref[torch.float64][1]):.2e}; {y_d:.2e})")
    assert float(ref[torch.float32][0].abs().max()) > 0 and float(ref[torch.float32][1].abs().max()) > 0
    assert bool(torch.isfinite(pg.grad).all()) and bool(torch.isfinite(dg.grad).all())
    assert e_p < GATE, e_p
    if (which, field) in F64_YARDSTICK_BLOCKS and not e_d < GATE:
        assert rel_err(dg.grad, ref[torch.float64][1]) <= 4 * y_d, (e_d, y_d)        # (this host's f32 reference flipped a ReLU)
    else:
        assert e_d < GATE, e_d
    # the decoder's own gradients came out of the same backward
    assert dec.blocks[3].weight.grad is not None and float(dec.blocks[3].weight.grad.abs().max()) > 0


# ---- (c), (d) the whole step ------------------------------------------------------------------------------------------------------------
def _ray_step(states, scene, latents, sigs, n_fine, grad, seed=7):
    from dfanerf import engine
    dev = torch.device("cuda")
    n = 64
    pix = _pixels(scene, n)
    r4, bounds = _jittered_rays(scene, pix, seed=seed)
    bg = (t(scene["bg"]).float() / 255.0).reshape(-1, 3)[pix].contiguous()
    rays = engine.pack_rays(*[x.to(dev) for x in r4]).requires_grad_(grad)
    fr = _rays_frame(n, 64, n_fine, near=5.0, far=6.0)
    r = _step(states, scene, latents, sigs, "f32", None, 64, n_fine, n, fr, bg.to(dev), rays=rays, bounds=bounds.to(dev))
    r["d_rays"] = None if rays.grad is None else rays.grad.detach().cpu().clone()
    return r, r4, bounds, bg


@pytest.mark.parametrize("n_fine", [0, 64])
def test_ray_gradient_of_the_step_vs_oracle_autograd(states, scene, latents, sigs, n_fine):
    """The inputs of test_jittered_rays_step_vs_oracle_autograd (64 jittered, rescaled rays, per-ray bounds), coarse and 64 + 64:
    rays.grad against torch CPU autograd through the oracle's render_fixed_samples at the kernel's own depths with the four ray blocks
    as leaves - per block (o_head, d_head, o_torso, d_torso) and as a whole tensor, at the d(signal) gate of that test - and every other
    output and gradient of the step bit for bit those of the step whose rays do not require grad.
    Measured (MI355X), against the f32 oracle: coarse o_head 2.7e-4, d_head 1.8e-4, o_torso 1.5e-6, d_torso 1.5e-6, whole 1.5e-4;
    64 + 64: 2.6e-4, 1.8e-4, 8.1e-5, 8.5e-5, whole 1.8e-4 (the f32 oracle's own error against float64: 5.6e-6 ... 7.4e-4)."""
    S = 64 + n_fine
    got, r4, bounds, bg = _ray_step(states, scene, latents, sigs, n_fine, True)
    plain, _, _, _ = _ray_step(states, scene, latents, sigs, n_fine, False)
    assert plain["d_rays"] is None and got["d_rays"] is not None and tuple(got["d_rays"].shape) == (64, 12)
    _assert_same_step(plain, got, "rays.requires_grad", n_fine > 0)
    z = got["z"] if n_fine else _per_ray_coarse_z(bounds, 64)
    zs, za = [t(v) for v in latents]
    refs = {}
    for dt in (torch.float32, torch.float64):
        P = {k: v.to(dt) for k, v in O.params_to_torch(states["decoder"]).items()}
        leaves = [x.clone().to(dt).requires_grad_(True) for x in r4]
        oh, oc = O.render_fixed_samples(P, *leaves, bg.to(dt), z.to(dt), zs.to(dt), za.to(dt), [sigs[0].to(dt), None],
                                        sigs[1][None].to(dt), 2)
        tgt = got["tgt"].to(dt)
        (((oh - tgt) ** 2).mean() + ((oc - tgt) ** 2).mean()).backward()
        refs[dt] = torch.cat([x.grad for x in leaves], 1)
    ref, ref64 = refs[torch.float32], refs[torch.float64]
    assert float(ref.abs().max()) > 0 and bool(torch.isfinite(got["d_rays"]).all())
    errs = {}
    for k, name in enumerate(("o_head", "d_head", "o_torso", "d_torso")):
        sl = slice(3 * k, 3 * k + 3)
        errs[name] = (rel_err(got["d_rays"][:, sl], ref[:, sl]), rel_err(got["d_rays"][:, sl], ref64[:, sl]), rel_err(ref[:, sl], ref64[:, sl]))
    errs["whole"] = (rel_err(got["d_rays"], ref), rel_err(got["d_rays"], ref64), rel_err(ref, ref64))
    print(f"ray gradient, {S} samples (vs the f32 oracle, vs float64, the f32 oracle's own error vs float64): " +
          ", ".join(f"{k} {a:.2e} {b:.2e} {c:.2e}" for k, (a, b, c) in errs.items()))
    bad = {k: v for k, v in errs.items() if not v[0] < GATE}
    assert not bad, bad


def test_ray_gradient_is_bit_reproducible(states, scene, latents, sigs):
    """two runs of the 64 + 64 step give identical d_rays (fixed-order sums in all three kernels, no atomics)"""
    a, _, _, _ = _ray_step(states, scene, latents, sigs, 64, True, seed=9)
    b, _, _, _ = _ray_step(states, scene, latents, sigs, 64, True, seed=9)
    assert a["d_rays"] is not None and float(a["d_rays"].abs().max()) > 0
    assert torch.equal(a["d_rays"], b["d_rays"])
    _assert_same_step(a, b, "two runs", True)


@pytest.mark.parametrize("n_coarse", [32, 64, 128])
def test_rays_grad_depths_are_the_forwards(n_coarse):
    """rays_grad_kernel rebuilds the coarse depths itself (csrc/dfn_train.hip: coarse_t / coarse_depth, next to the compositing
    backward's own statement of the same arithmetic).  n_coarse rays, ray r with dL/d point = (1, 0, 0) at its sample r and zero
    elsewhere: the direction block then holds sum_j z_j g_x_j = z_r exactly, which must equal near (1 - t) + far t of that ray's bounds
    (the depths the forward is pinned to, test_gpu_train_rays.py) BIT FOR BIT - with per-ray bounds and with the frame's pair."""
    from dfanerf import engine
    from dfanerf._lib import check, lib
    dev, n = "cuda", n_coarse
    rs = np.random.RandomState(5 + n_coarse)
    rays = t(_random_rays(rs, n)).to(dev).contiguous()
    bounds = t(np.stack([0.3 + rs.uniform(0, 0.05, n), 0.9 - rs.uniform(0, 0.05, n)], 1).astype(np.float32))
    gx = torch.zeros(n, n_coarse, 3)
    gx[torch.arange(n), torch.arange(n), 0] = 1.0
    gx, zero, dn = gx.to(dev).contiguous(), torch.zeros(n * n_coarse, 3, device=dev), torch.zeros(n, 2, device=dev)
    junk = np.full((4, 4), 7.5, np.float32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for bd, near, far in ((bounds, 5.0, 6.0), (None, 0.31, 0.87)):
        fr = engine.make_frame(3, 5, 1.0, -2.0, 9.0, junk, junk, near, far, 1e10, 11, n, n_coarse, 0, 2, True)
        out = torch.full((n, 12), float("nan"), device=dev)
        BD = None if bd is None else bd.to(dev).contiguous()
        check(lib.dfn_rays_grad(0, C.byref(fr), rays.data_ptr(), None if BD is None else BD.data_ptr(), None, None, gx.data_ptr(),
                                zero.data_ptr(), zero.data_ptr(), zero.data_ptr(), dn.data_ptr(), out.data_ptr(), st), "dfn_rays_grad")
        torch.cuda.synchronize()
        z = _per_ray_coarse_z(bd, n_coarse) if bd is not None else O.coarse_z(near, far, n_coarse)[None].expand(n, n_coarse)
        want = z[torch.arange(n), torch.arange(n)]
        got = out.cpu()
        assert torch.equal(got[:, 3], want), float((got[:, 3] - want).abs().max())
        assert torch.equal(got[:, 0], torch.ones(n)) and float(got[:, [1, 2, 4, 5]].abs().max()) == 0.0
        assert float(got[:, 6:].abs().max()) == 0.0


# ---- (e) an end-to-end pose fit ----------------------------------------------------------------------------------------------------------
# the same fit through the oracle's autograd on the CPU (python tests/ray_grad_fit.py): loss and pose error |q| at the start and after
# the 40 steps.  The library must reach at least half of each reduction.
ORACLE_FIT = {"loss": (4.463927e-03, 4.496461e-05), "err": (4.597825e-03, 2.162964e-03)}


def test_pose_fit_through_pinhole_rays(states, scene, latents, sigs):
    """256 pixels, targets rendered at the true poses, start = FIT.START (a translation offset on both origins, a small rotation of the
    head pose), 40 Adam steps on the 6 + 3 parameters through training.pinhole_rays -> render_train(rays=...): the loss and the pose
    error fall by at least half of what the same fit reaches through the oracle's autograd."""
    from dfanerf import engine, training
    dev = torch.device("cuda")
    n = FIT.N_PIX
    dec = _decoder(states, dev)
    buf = training.TrainBuffers("f32", n, dev)
    fr = _rays_frame(n, 64, 0, near=FIT.NEAR, far=FIT.FAR)
    bg = (t(scene["bg"]).float() / 255.0).reshape(-1, 3)[FIT.pixels(scene)].contiguous().to(dev)
    zs, za = [t(v).to(dev) for v in latents]
    sh, st = [x.to(dev) for x in sigs]

    def render(rays):        # (the nine parameters and pinhole_rays live on the CPU: the rays cross to the device inside the graph)
        dec.zero_grad(set_to_none=True)
        return training.render_train(dec, buf, fr, bg, None, sh, st, zs[0, :2], za[0, :2], rays=rays.to(dev))
    losses, errs = FIT.fit(scene, render)
    o = ORACLE_FIT
    print(f"pose fit: loss {losses[0]:.4e} -> {losses[-1]:.4e} (oracle {o['loss'][0]:.4e} -> {o['loss'][1]:.4e}), pose error "
          f"{errs[0]:.4e} -> {errs[-1]:.4e} (oracle {o['err'][0]:.4e} -> {o['err'][1]:.4e})")
    assert np.isfinite(losses).all() and np.isfinite(errs).all()
    assert o["loss"][1] < o["loss"][0] and o["err"][1] < o["err"][0]
    assert errs[0] == pytest.approx(o["err"][0], rel=1e-5)            # the same start
    assert losses[0] - losses[-1] >= 0.5 * (o["loss"][0] - o["loss"][1]), (losses[0], losses[-1])
    assert errs[0] - errs[-1] >= 0.5 * (o["err"][0] - o["err"][1]), (errs[0], errs[-1])
