"""Two-field rendering and training where the two fields really BLEND, on the GPU, against the CPU oracle.

Decoder: tests/blend_scene.py (the fixtures' network with the torso's input matrices x 0.03 and sigma_out.bias - 18): translucent
composites on all 93 rays, 28 of them with both fields carrying weight, 26 different argmax bins of the coarse composite weights,
the composite loss's gradient almost entirely behind the first 4 samples (tests/test_blend_scene_host.py asserts these with the
oracle).  93 rays of frame 2, golden G7's conditioning; sample pairs (32, 0), (64, 0), (32, 32), (32, 64), (64, 128).

  a. exact tiers (f32; f16x3) against the oracle at the kernel's own depths: the project's gates (rgb 5e-5, weight sums 2e-6, depths
     within one coarse bin) and EVERY weight within four times the oracle's own float64-vs-float32 difference (W_GATE below: the
     project's per-weight 2e-6 is under the reference's own f32 error on translucent rays);
  b. the sampler + rank merge, bit for bit, fed the kernel's own coarse weights: many different inverse CDFs here;
  c. opacity and expected depth, exact tier, against the oracle (S 2e-6, z_far S 2e-6); the aux call's RGB is the plain call's;
  d. the variants agree: u8 epilogue, caller-supplied rays, the recording forward;
  e. the 16-bit tiers, gated by a ROUNDING MODEL computed on the CPU from the reference alone (blend_scene.model_fields: every GEMM
     operand rounded to the tier's type, nearest-even, everything else exact): per image, rms error of the kernel against the exact
     oracle <= 2 x the model's, largest per-ray error <= 3 x the model's.  The factors cover what the model does not have - f32
     accumulation order (about a fifth of the rounding error on the head field) and the hardware sine; measured on the CPU, their
     sum is about 1.2;  the f16 tier's accuracy guard on this decoder reports what it measures;
  f. the training step, exact tier, coarse and hierarchical (64 + 64), against oracle autograd with
     test_training_step_full_size_vs_oracle_autograd's gates; the torso-only tensors' reference gradients are not zero; the
     compositing backward alone on the step's own recorded samples.

No gate here was chosen after looking at the kernel's output: each is an existing project gate, derives from the rounding model, or is
four times the oracle's float64-vs-float32 difference."""
import ctypes as C

import numpy as np
import pytest
import torch

import blend_scene as B
import dfa_oracle as O
import test_gpu_samples as TS
from dfanerf import synth

pytestmark = pytest.mark.gpu

N_RAYS, FRAME = B.N_RAYS, B.FRAME
ALL_PAIRS = [(32, 0), (64, 0), (32, 32), (32, 64), (64, 128)]
HIER_PAIRS = [(32, 32), (32, 64), (64, 128)]
t = B.t


@pytest.fixture(scope="module")
def eng():
    from dfanerf import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope="module")
def bstates(states):
    return B.blend_states(states)


@pytest.fixture(scope="module")
def packed(eng, bstates):
    flat = eng.flatten_state(bstates["decoder"], "cuda")
    cache = {}

    def get(tier):
        if tier not in cache:
            cache[tier] = eng.PackedDecoder(flat, tier)
        return cache[tier]
    return get


@pytest.fixture(scope="module")
def cond(golden, latents):
    return B.conditioning(golden("g7_frame_coarse"), latents)


@pytest.fixture(scope="module")
def pix(scene):
    return B.ray_indices(scene)


@pytest.fixture(scope="module")
def bg(scene):
    return (t(scene["bg"]).float() / 255.0).reshape(-1, 3).cuda()


@pytest.fixture(scope="module")
def orc(scene, bstates, latents, golden, pix):
    return B.Oracle(scene, bstates["decoder"], latents, golden("g7_frame_coarse"), pix)


def _render(eng, pk, cnd, scene, bg, pix, nc, nf, fields, **kw):
    return TS._render(eng, pk, cnd, scene, bg, pix, nc, nf, fields, **kw)


def _np(outs):
    return [None if o is None else o.cpu().numpy() for o in outs]


# ---- a ------------------------------------------------------------------------------------------------------------------------------
# The per-weight gate.  The project's 2e-6 (test_render_coarse_f32_vs_reference_golden) is tighter than the REFERENCE'S OWN float32
# error on this scene: the oracle's arithmetic in float64 against the same oracle in float32, same decoder, same depths, differs by up
# to W_F64[image] in a single weight (largest of the five pairs, at 32 + 0; tests/test_blend_scene_host.py re-measures it) - a
# translucent ray's transmittance carries the densities' f32 error (2e-4 in a raw sigma of tens) through every sample, an opaque
# ray's does not.  That is more than half the gate, so the gate for this scene is four times the reference's own difference.
W_GATE = {name: 4.0 * v for name, v in B.W_F64.items()}                     # head 2.0e-5, com 7.1e-6


@pytest.mark.parametrize("tier,nc,nf", [("f32", nc, nf) for nc, nf in ALL_PAIRS] + [("f16x3", 32, 64), ("f16x3", 64, 0)])
def test_exact_tiers_vs_oracle_at_the_kernels_depths(eng, packed, cond, scene, bg, pix, orc, tier, nc, nf):
    """test_gpu_samples._f32_gates on the blend decoder, two fields, plus every single weight of both images"""
    rh, rc, wh, wc, z = _np(_render(eng, packed(tier), cond, scene, bg, pix, nc, nf, 2, want_weights=True, want_z=True))
    near, far = np.float32(scene["near"]), np.float32(scene["far"])
    assert z.shape == (N_RAYS, nc + nf) and (np.diff(z, axis=1) >= 0).all()
    assert (z[:, 0] == near).all() and (z[:, -1] == far).all()
    aux = orc.render(nc, nf, 2)[2]
    dz = np.abs(z - (aux["z_all"] if nf else aux["z_coarse"]).numpy()).max()
    oh, owh, oc, owc = [x.numpy() for x in orc.at(z)]
    e = {"rgb_head": np.abs(rh - oh).max(), "rgb_com": np.abs(rc - oc).max(), "w_head": np.abs(wh - owh).max(),
         "w_com": np.abs(wc - owc).max(), "sum w_head": np.abs(wh.sum(1) - 1.0).max(), "sum w_com": np.abs(wc.sum(1) - 1.0).max()}
    print(f"{tier} {nc}+{nf}: max |z - oracle z| {dz:.3e} (bin {(far - near) / (nc - 1):.3e}); " +
          ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    acc = owc[:, :-1].sum(1)
    assert ((acc >= 0.1) & (acc <= 0.9)).sum() >= 60                       # the composite these depths give is translucent
    assert dz <= (float(far) - float(near)) / (nc - 1) * 1.001
    np.testing.assert_allclose(wh.sum(1), 1.0, atol=2e-6)
    np.testing.assert_allclose(wc.sum(1), 1.0, atol=2e-6)
    np.testing.assert_allclose(rh, oh, atol=5e-5, rtol=0)
    np.testing.assert_allclose(rc, oc, atol=5e-5, rtol=0)
    np.testing.assert_allclose(wh, owh, atol=W_GATE["head"], rtol=0)
    np.testing.assert_allclose(wc, owc, atol=W_GATE["com"], rtol=0)


# ---- b ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("fields", [1, 2])
@pytest.mark.parametrize("nc,nf", HIER_PAIRS + [(64, 32)])
def test_sampler_is_bit_exact_given_the_coarse_weights(eng, packed, cond, scene, bg, pix, tier, fields, nc, nf):
    """test_gpu_samples.test_sampler_is_bit_exact_given_the_coarse_weights where the composite's coarse weights peak in more than 20
    different bins (two fields) and the head image is translucent on more rays (one field)"""
    pk = packed(tier)
    out = _render(eng, pk, cond, scene, bg, pix, nc, 0, fields, want_weights=True, want_z=True)
    w = (out[3] if fields == 2 else out[2]).cpu()
    z = out[-1].cpu()
    assert np.array_equal(z.numpy(), O.coarse_z(scene["near"], scene["far"], nc)[None].expand(N_RAYS, nc).numpy())
    inner = w[:, 1:-1].numpy()
    assert len(np.unique(inner.argmax(1))) >= nc // 4                        # (the kernel's own weights: not one inverse CDF)
    z_all = _render(eng, pk, cond, scene, bg, pix, nc, nf, fields, want_z=True)[-1].cpu()
    assert z_all.shape == (N_RAYS, nc + nf)
    z_mid = .5 * (z[..., 1:] + z[..., :-1])
    z_f = O.sample_pdf(z_mid, w[..., 1:-1], nf, det=True, fixed_order=True)
    want, _ = torch.sort(torch.cat([z, z_f], -1), -1)
    assert fields == 1 or len(np.unique(z_f.numpy(), axis=0)) == N_RAYS       # (head image: its empty rays look alike)
    assert np.array_equal(z_all.numpy(), want.numpy()), float((z_all - want).abs().max())


# ---- c ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc,nf", [(32, 0), (32, 32)])
def test_aux_against_the_oracle_exact_tier(eng, packed, cond, scene, bg, pix, orc, nc, nf):
    pk, S = packed("f32"), nc + nf
    rh, rc, _, _, z = _np(_render(eng, pk, cond, scene, bg, pix, nc, nf, 2, want_weights=True, want_z=True))
    ah_rgb, ac_rgb, ah, ac = _np(_render(eng, pk, cond, scene, bg, pix, nc, nf, 2, want_aux=True))
    assert np.array_equal(ah_rgb, rh) and np.array_equal(ac_rgb, rc) and np.isfinite(rc).all() and float(rc.std()) > 0.01
    _, owh, _, owc = [x.double().numpy() for x in orc.at(z)]
    z64, z_far = z.astype(np.float64), float(scene["far"])
    for name, a, w in (("head", ah, owh), ("com", ac, owc)):
        acc, dep = w[:, :-1].sum(1), (w[:, :-1] * z64[:, :-1]).sum(1)          # concate_bg: FG = every sample but the last
        e_acc, e_dep = np.abs(a[:, 0] - acc).max(), np.abs(a[:, 1] - dep).max()
        print(f"{nc}+{nf}, {name}: max |acc - oracle| {e_acc:.2e} (gate {S * 2e-6:.1e}), max |depth - oracle| {e_dep:.2e} "
              f"(gate {z_far * S * 2e-6:.1e}); acc in [{acc.min():.4f}, {acc.max():.4f}]")
        assert a.shape == (N_RAYS, 2) and a.dtype == np.float32
        assert e_acc <= S * 2e-6 and e_dep <= z_far * S * 2e-6, (name, e_acc, e_dep)
        if name == "com":
            assert ((acc >= 0.1) & (acc <= 0.9)).sum() >= 60


# ---- d ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["f32", "f16"])
def test_u8_epilogue_equals_to8b_of_the_float_render_32_plus_64(eng, packed, cond, scene, bg, pix, tier):
    sa, stt, zs, za = cond
    pk = packed(tier)
    bias = pk.fold(sa, stt, zs, za)
    px = t(pix).cuda()
    for fr, kw in ((TS._frame(eng, scene, 32, 64, 2, n=N_RAYS, begin=(scene["H"] // 2) * scene["W"] + 17), {}),
                   (TS._frame(eng, scene, 32, 64, 2, n=N_RAYS), {"pix_index": px})):
        f_h, f_c = eng.render(pk, bias, fr, bg, **kw)[:2]
        u_h, u_c = eng.render_u8(pk, bias, fr, bg, **kw)
        assert u_h.dtype == torch.uint8 and tuple(u_h.shape) == (N_RAYS, 3) and float(f_c.std()) > 0.01
        assert torch.equal(u_h, eng.to8b(f_h)) and torch.equal(u_c, eng.to8b(f_c))


@pytest.mark.parametrize("tier", ["f32", "f16"])
def test_rays_launch_fed_the_frames_own_rays_equals_the_plain_launch_32_plus_64(eng, packed, cond, scene, bg, pix, tier):
    sa, stt, zs, za = cond
    pk = packed(tier)
    plain = _render(eng, pk, cond, scene, bg, pix, 32, 64, 2, want_weights=True, want_z=True)
    geo = (scene["H"], scene["W"], scene["focal"])
    sel = t(pix).long().cuda()
    o_h, d_h = eng.get_rays(*geo, scene["poses"][FRAME], scene["cx"], scene["cy"])
    o_t, d_t = eng.get_rays(*geo, scene["pose_body"], scene["cx"], scene["cy"])
    rays = eng.pack_rays(*[x.reshape(-1, 3)[sel].contiguous() for x in (o_h, d_h, o_t, d_t)])
    junk = np.full((4, 4), 7.5, np.float32)              # a rays launch ignores the frame's poses and intrinsics
    fr = eng.make_frame(3, 5, 1.0, -2.0, 9.0, junk, junk, scene["near"], scene["far"], ray_begin=11, ray_count=N_RAYS, n_coarse=32,
                        n_fine=64, fields=2)
    got = eng.render(pk, pk.fold(sa, stt, zs, za), fr, bg[sel].contiguous(), rays=rays, want_weights=True, want_z=True)
    assert len(got) == len(plain) == 5 and got[-1].shape == (N_RAYS, 96) and float(plain[1].std()) > 0.01
    for k, (a, b) in enumerate(zip(got, plain)):
        assert torch.equal(a, b), (tier, k, float((a - b).abs().max()))


def test_recording_forward_equals_the_inference_kernel_32_plus_64(eng, bstates, cond, scene, bg, pix):
    """(the recorder is the exact tier's: dfn_train_fwd_hier, f32; the f16 tier is inference only)"""
    TS.test_recording_forward_equals_the_inference_kernel(eng, bstates, cond, scene, bg, pix, 32, 64)


# ---- e ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["f16", "bf16"])
@pytest.mark.parametrize("nc,nf", [(32, 0), (32, 32)])
def test_16_bit_tiers_within_the_rounding_models_error(eng, packed, cond, scene, bg, pix, orc, tier, nc, nf):
    rh, rc, z = _np(_render(eng, packed(tier), cond, scene, bg, pix, nc, nf, 2, want_z=True))
    assert np.isfinite(rh).all() and np.isfinite(rc).all()
    exact = orc.at(z)
    model = orc.integrate(z, *B.model_fields(orc, z, tier))
    for name, got, k in (("head", rh, 0), ("com", rc, 2)):
        ref = exact[k].numpy()
        m_rms, m_top, m_db = B.image_errors(model[k].numpy(), ref)
        k_rms, k_top, k_db = B.image_errors(got, ref)
        print(f"{tier} {nc}+{nf} rgb_{name}: model rms {m_rms:.3e}, largest per-ray {m_top:.3e}, {m_db:.1f} dB | kernel rms {k_rms:.3e}, "
              f"largest per-ray {k_top:.3e}, {k_db:.1f} dB | ratios {k_rms / m_rms:.2f} (gate 2), {k_top / m_top:.2f} (gate 3)")
        assert m_rms > 0 and k_rms <= 2.0 * m_rms, (tier, nc, nf, name, k_rms, m_rms)
        assert k_top <= 3.0 * m_top, (tier, nc, nf, name, k_top, m_top)


def test_f16_accuracy_guard_reports_what_it_measures(eng, bstates, cond, scene, latents, bg):
    """the f16 tier's accuracy guard (dfanerf/f16guard.py) on the blend decoder at 32 + 32: its statistics are the PSNR of the f16
    images against the exact tier's on its own calibration sample, recomputed here; its verdict is the comparison of that figure
    with its gate (49.4 dB for a 30-dB model).  Whether the tier passes on this decoder is a property of the tier, not asserted."""
    from dfanerf import f16guard, run_nerf
    from dfanerf.decoder import Decoder
    dev = torch.device("cuda")
    dec = Decoder(z_dim=256, hidden_size=256, dim_signal=96, use_deformation_field=True)
    dec.load_state_dict({k: t(v) for k, v in bstates["decoder"].items()})
    dec.to(dev)
    args = run_nerf.config_parser().parse_args(
        "--expname t --concate_bg --dim_signal=96 --n_object=1 --use_deformation_field --hierarchical --N_samples 32 "
        "--N_importance 32 --hip_tier f16".split())
    zs, za = [t(v).to(dev) for v in latents]
    plate = (t(scene["bg"]).float() / 255.0).to(dev)
    R = run_nerf.FrameRenderer(dec, zs, za, plate, [scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"]], scene["near"],
                               scene["far"], args)
    sh, st = t(cond[0]).to(dev), t(cond[1]).to(dev)
    poses, n_rays, refused = list(scene["poses"][:4]), 256, None
    try:
        R.check_f16_accuracy(poses, scene["pose_body"], lambda k: (sh, st), n_rays=n_rays)
    except f16guard.F16AccuracyError as e:
        refused = str(e)
    stats = R.decoder.packed("f16").f16_accuracy
    gate = f16guard.psnr_gate(f16guard.DEFAULT_MODEL_PSNR)
    # the same sample, rendered here: the guard's pixel draws are torch.randperm of a CPU generator seeded 0, one per frame
    gen = torch.Generator(device="cpu").manual_seed(0)
    mses = {"head": [], "com": []}
    for k in range(len(poses)):
        px = torch.randperm(scene["H"] * scene["W"], generator=gen)[:n_rays].to(torch.int32).to(dev)
        img = {}
        for tier in ("f16", "f32"):
            pk = R.decoder.packed(tier)
            fr = eng.make_frame(scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"], poses[k], scene["pose_body"],
                                scene["near"], scene["far"], ray_count=n_rays, n_coarse=32, n_fine=32, fields=2)
            img[tier] = eng.render(pk, pk.fold(sh, st, zs[0], za[0]), fr, bg, pix_index=px)
        for i, name in enumerate(("head", "com")):
            mses[name].append(float(((img["f16"][i].double() - img["f32"][i].double()) ** 2).mean()))
    ok = True
    for name in ("head", "com"):
        s = stats[name]
        want, worst = -10 * np.log10(np.mean(mses[name])), -10 * np.log10(np.max(mses[name]))
        print(f"f16 accuracy guard on the blend decoder, 32+32, {name}: {s['psnr_db']:.2f} dB (worst frame {s['worst_block_db']:.2f}), "
              f"recomputed {want:.2f} / {worst:.2f}; gate {gate:.2f} dB")
        assert s["n_rays"] == n_rays * len(poses) and abs(s["psnr_db"] - want) < 1e-6 and abs(s["worst_block_db"] - worst) < 1e-6
        ok = ok and s["psnr_db"] >= gate and s["worst_block_db"] >= gate - f16guard.BLOCK_SLACK_DB
    print("verdict: " + ("accepted" if refused is None else "refused: " + refused))
    assert ok == (refused is None)
    assert refused is None or "loses the accuracy clause" in refused


# ---- f ------------------------------------------------------------------------------------------------------------------------------
def _oracle_step(bstates, scene, latents, sel, tgt_h, tgt_c, step, z=None):
    """the reference's step (MAIN:779-907; O.train_loss) under torch CPU autograd with every parameter of all five networks a leaf;
    z: the depths to render at (the hierarchical step's own merged depths: constants there and here) instead of the coarse ones"""
    keep = torch.get_num_threads()
    torch.set_num_threads(min(16, keep))
    try:
        H, W = scene["H"], scene["W"]
        zs, za = [t(v) for v in latents]
        auds, exps, poses = t(scene["aud"]), t(scene["exp"]), t(scene["poses"])
        allp = {tag: {k: t(v).clone().requires_grad_(True) for k, v in st.items()} for tag, st in bstates.items()}
        nets = {k: v for k, v in allp.items() if k != "decoder"}
        bgi = t(scene["bg"]).float() / 255.0
        if z is None:
            loss, lh, lc = O.train_loss(allp["decoder"], nets, t(sel), H, W, scene["focal"], scene["cx"], scene["cy"], poses[3], poses[0],
                                        bgi, tgt_h, tgt_c, 0.3, 0.9, zs, za, auds, exps, poses, 3, step, 300000, 4, 8, auds.shape[0])
        else:
            sig = O.encode_signal(nets, auds, exps, 3, step, 300000, 4, auds.shape[0])
            sigt = O.encode_signal_torso(nets, poses, 3, step, 300000, 8, auds.shape[0])
            o_h, d_h = O.get_rays(H, W, scene["focal"], poses[3][:3, :4], scene["cx"], scene["cy"])
            o_t, d_t = O.get_rays(H, W, scene["focal"], poses[0][:3, :4], scene["cx"], scene["cy"])
            ys, xs = t(sel[:, 0]), t(sel[:, 1])
            rh, rc = O.render_fixed_samples(allp["decoder"], o_h[ys, xs], d_h[ys, xs], o_t[ys, xs], d_t[ys, xs], bgi[ys, xs], z, zs, za,
                                            sig, sigt, 2)
            lh, lc = O.img2mse(rh, tgt_h[ys, xs]), O.img2mse(rc, tgt_c[ys, xs])
            loss = lc + lh
        loss.backward()
        return ([loss.item(), lh.item(), lc.item()],
                {f"{tag}/{k}": (None if v.grad is None else v.grad.clone()) for tag, prm in allp.items() for k, v in prm.items()})
    finally:
        torch.set_num_threads(keep)


def _composite_bwd_alone(scene, buf, fr, pix, bgi, d_h, d_c, sel, n, S, n_fine):
    """dfn_composite_bwd / dfn_composite_bwd_hier on the step's own recorded samples against autograd through integrate_fields, at
    test_composite_backward_vs_autograd's tolerance"""
    from dfanerf._lib import check, lib
    H, W = scene["H"], scene["W"]
    ds = torch.full((n, S, 8), float("nan"), device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if n_fine:
        check(lib.dfn_composite_bwd_hier(C.byref(fr), p(pix), p(bgi), None, p(buf.samples), p(buf.z_all), p(buf.ranks), p(d_h), p(d_c),
                                         p(ds), st), "dfn_composite_bwd_hier")
    else:
        check(lib.dfn_composite_bwd(C.byref(fr), p(pix), p(bgi), None, p(buf.samples), p(d_h), p(d_c), p(ds), st), "dfn_composite_bwd")
    torch.cuda.synchronize()
    sm = buf.samples.cpu().reshape(n, S, 8).clone().requires_grad_(True)
    assert bool(torch.isfinite(sm).all())
    if n_fine:
        z = buf.z_all.cpu()
        idx = buf.ranks.cpu().long()                                          # ranks[r, e] = merged position of evaluated point e
        inv = torch.empty_like(idx)
        inv.scatter_(1, idx, torch.arange(S)[None].expand(n, S))
        merged = torch.gather(sm, 1, inv[..., None].expand(n, S, 8))
    else:
        z, merged = O.coarse_z(0.3, 0.9, 64)[None].expand(n, 64), sm
    _, dir_h = O.get_rays(H, W, scene["focal"], scene["poses"][3][:3, :4], scene["cx"], scene["cy"])
    _, dir_t = O.get_rays(H, W, scene["focal"], scene["poses"][0][:3, :4], scene["cx"], scene["cy"])
    ys, xs = t(sel[:, 0]), t(sel[:, 1])
    rh, _, rc, w_c = O.integrate_fields(z, dir_h[ys, xs], dir_t[ys, xs], merged[..., 0], merged[..., 1:4], merged[..., 4],
                                        merged[..., 5:8], (t(scene["bg"]).float() / 255.0)[ys, xs])
    ((rh * d_h.cpu()).sum() + (rc * d_c.cpu()).sum()).backward()
    got, ref = ds.cpu().numpy(), sm.grad.numpy()
    acc = w_c.detach()[:, :-1].sum(1).numpy()
    deep = np.abs(ref[:, 4:, [0, 4]]).sum() / np.abs(ref[..., [0, 4]]).sum()
    print(f"    compositing backward alone: max |d samples - autograd| {np.abs(got - ref).max():.2e} (max |ref| {np.abs(ref).max():.2e}); "
          f"{int(((acc >= 0.1) & (acc <= 0.9)).sum())} of {n} composites translucent")
    assert np.isfinite(got).all() and np.abs(ref[..., 4]).max() > 0 and np.abs(ref[..., 0]).max() > 0
    np.testing.assert_allclose(got, ref, atol=2e-5 * np.abs(ref).max(), rtol=2e-4)
    return deep


@pytest.mark.parametrize("n_fine", [0, 64])
def test_training_step_vs_oracle_autograd(bstates, scene, latents, n_fine):
    """test_training_step_full_size_vs_oracle_autograd's procedure and gates on the blend decoder: 256 distinct pixels, both fields,
    all five networks, smoothed signal branch (step 300000), tier f32; coarse (64 samples) and hierarchical (64 + 64: the oracle
    renders at the step's own merged depths, which are held against the oracle's row-H depths as test_gpu_train_hier does)."""
    import test_gpu_train as TT
    from dfanerf import engine, nets, run_nerf, training
    dev = torch.device("cuda")
    step, n, S = 300000, 256, 64 + n_fine
    H, W = scene["H"], scene["W"]
    flat_px = np.random.RandomState(11).permutation(H * W)[:n]
    sel = np.stack([flat_px // W, flat_px % W], axis=1).astype(np.int64)
    tgt_h = t(synth.synth_tensor(0, "g8/th", (H, W, 3), 0.5)) + 0.5
    tgt_c = t(synth.synth_tensor(0, "g8/tc", (H, W, 3), 0.5)) + 0.5
    mods = TT._modules(bstates, dev)
    args = run_nerf.config_parser().parse_args(
        "--expname t --concate_bg --N_rand=256 --sample_rate=0 --smo_size=4 --smo_torse_size 8 --use_et_embed "
        "--dim_signal=96 --dim_aud=96 --n_object=1 --use_deformation_field --noexp_iters 400000".split())
    ds = [{"auds": t(scene["aud"]).to(dev), "exp": t(scene["exp"]).to(dev), "poses": t(scene["poses"]).to(dev),
           "bc_img": (t(scene["bg"]).float() / 255.0).to(dev), "hwfcxy": [H, W, scene["focal"], scene["cx"], scene["cy"]],
           "near": 0.3, "far": 0.9}]
    zs, za = [t(v).to(dev) for v in latents]
    embed_fn, _ = nets.get_embedder(3, 0)
    buf = training.TrainBuffers("f32", n, dev, n_fine=n_fine)
    buf.signal_trainer = training.SignalTrainer(mods["AudNet"], mods["ExpNet"], mods["AudAttNet"], mods["PoseAttNet"],
                                                ds[0]["auds"], ds[0]["exp"], ds[0]["poses"])
    ys, xs = t(sel[:, 0]).to(dev), t(sel[:, 1]).to(dev)
    th, tc = tgt_h.to(dev)[ys, xs], tgt_c.to(dev)[ys, xs]
    loss, lh, lc, rgb_h, rgb_c = run_nerf.train_step_loss_hip(mods, ds, 0, 3, sel, th, tc, zs, za, step, args, scene["aud"].shape[0],
                                                              embed_fn, ds[0]["poses"][0], buf)
    loss.backward()
    torch.cuda.synchronize()
    z = None
    if n_fine:
        z = buf.z_all.cpu()
        assert bool((z[:, 1:] >= z[:, :-1]).all()) and float((z[:, -1] - 0.9).abs().max()) == 0.0
    ref_loss, ref_g = _oracle_step(bstates, scene, latents, sel, tgt_h, tgt_c, step, z)
    np.testing.assert_allclose([loss.item(), lh.item(), lc.item()], ref_loss, rtol=3e-5)
    worst, worst_dir, worst_cos, seen = 0.0, 0.0, 1.0, set()
    for tag, m in mods.items():
        for k, p in m.named_parameters():
            ref = ref_g[f"{tag}/{k}"]
            rn = 0.0 if ref is None else float(ref.double().norm())
            if tag == "decoder" and k.startswith(B.TORSO_ONLY):
                assert rn > 0.0, k                                        # the torso's own tensors take part: never skipped below
                seen.add(k)
            if rn == 0.0:
                assert p.grad is None or float(p.grad.abs().max()) <= 1e-12, (tag, k)
                continue
            g = p.grad.detach().cpu()
            gn = float(g.double().norm())
            worst = max(worst, abs(gn - rn) / rn)
            assert abs(gn - rn) <= 1e-3 * rn + 1e-9, (tag, k, gn, rn)
            d = float((g - ref).double().norm()) / rn
            worst_dir = max(worst_dir, d)
            cos = float(g.double().reshape(-1) @ ref.double().reshape(-1)) / (gn * rn)
            worst_cos = min(worst_cos, cos)
            assert cos >= 1.0 - 1e-6, (tag, k, cos)
            assert d <= 5e-4, (tag, k, d)
            gs, rs_ = g.reshape(-1), ref.reshape(-1)
            stride = max(1, gs.numel() // 8)
            rms = rn / np.sqrt(gs.numel())
            np.testing.assert_allclose(gs[::stride][:8].numpy(), rs_[::stride][:8].numpy(), rtol=2e-2, atol=1e-3 * rms + 1e-9)
    assert len(seen) >= 20 and {"fc_in_torso.weight", "fc_p_skips_torso.0.weight", "deform_net.out_embed.weight"} <= seen, sorted(seen)
    print(f"blend step, f32, 64+{n_fine}: loss {loss.item():.6f} (oracle {ref_loss[0]:.6f}), worst relative gradient-norm error {worst:.2e}, "
          f"worst whole-tensor error {worst_dir:.2e}, worst cosine {worst_cos:.8f}")
    # the compositing backward alone, on this step's recorded samples and its d loss / d rgb
    fr = engine.make_frame(H, W, scene["focal"], scene["cx"], scene["cy"], scene["poses"][3], scene["poses"][0], 0.3, 0.9, 1e10, 0, n,
                           64, n_fine, 2, True)
    pixd = t((sel[:, 0] * W + sel[:, 1]).astype(np.int32)).to(dev)
    bgi = ds[0]["bc_img"].reshape(-1, 3).contiguous()
    d_h = (2.0 * (rgb_h.detach() - th) / (3 * n)).float().contiguous()
    d_c = (2.0 * (rgb_c.detach() - tc) / (3 * n)).float().contiguous()
    deep = _composite_bwd_alone(scene, buf, fr, pixd, bgi, d_h, d_c, sel, n, S, n_fine)
    print(f"    share of the step's |d loss / d sigma| behind the first 4 samples: {deep:.3f}")
    if n_fine == 0:
        assert deep >= 0.5
    else:
        with torch.no_grad():
            P = O.params_to_torch(bstates["decoder"])
            onets = {k: O.params_to_torch(v) for k, v in bstates.items() if k != "decoder"}
            auds, exps, poses = t(scene["aud"]), t(scene["exp"]), t(scene["poses"])
            sig = O.encode_signal(onets, auds, exps, 3, step, 300000, 4, auds.shape[0])
            sigt = O.encode_signal_torso(onets, poses, 3, step, 300000, 8, auds.shape[0])
            o_h, d_hh = O.get_rays(H, W, scene["focal"], poses[3][:3, :4], scene["cx"], scene["cy"])
            o_t, d_tt = O.get_rays(H, W, scene["focal"], poses[0][:3, :4], scene["cx"], scene["cy"])
            yc, xc = t(sel[:, 0]), t(sel[:, 1])
            _, _, aux = O.render_rays_chunk(P, o_h[yc, xc], d_hh[yc, xc], o_t[yc, xc], d_tt[yc, xc], (t(scene["bg"]).float() / 255.0)[yc, xc],
                                            0.3, 0.9, t(latents[0]), t(latents[1]), sig, sigt, 64, n_fine, 2, return_aux=True)
        assert float((z - aux["z_all"]).abs().max()) < 0.6 / 63 * 1.001
