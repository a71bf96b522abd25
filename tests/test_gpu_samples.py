"""The hierarchical mode of the fused renderer at the sample counts next to 64 + 64 | 128: (n_coarse, n_fine) = (32, 32), (32, 64)
and (64, 32), on the GPU, through the C ABI.  The fine sampler is a 64-lane wave program with one coarse sample per lane: at 32
coarse samples the upper half of the wave owns none, at 32 fine samples half the wave owns no fine sample.

  1. the sampler + rank merge, bit for bit, given the kernel's own coarse weights (oracle sample_pdf in the documented sum order);
  2. decoder and compositing at the kernel's own depths against the CPU oracle, f32 tier (the gates of
     test_gpu_parity.test_render_hierarchical_64_fine_vs_oracle);  3. the same for the f16x3 tier;
  4. the render variants: u8 epilogue, the 128-wide program, caller-supplied rays, the aux outputs;
  5. the recording forward (dfn_train_fwd_hier) against the inference kernel, bit for bit;
  6. both f16 guards and the command line at 32 + 64;  7. refused pairs launch nothing.

93 rays everywhere: no multiple of 8 or 4, so the last workgroup has idle waves in every tier.  Scene, weights and signals: golden
G7's (tests/test_gpu_parity.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import dfa_oracle as O
from dfanerf import synth
from test_gpu_driver import COMMON, F_VAL, H, W, _run, dataset      # noqa: F401  (its synthetic dataset on disk, as a fixture of this module too)

pytestmark = pytest.mark.gpu

PAIRS = [(32, 32), (32, 64), (64, 32)]
N_RAYS = 93
FRAME = 2


def t(x):
    return torch.from_numpy(np.asarray(x))


@pytest.fixture(scope="module")
def eng():
    from dfanerf import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope="module")
def packed(eng, states):
    flat = eng.flatten_state(states["decoder"], "cuda")
    return {tier: eng.PackedDecoder(flat, tier) for tier in ("f32", "f16", "f16x3", "bf16")}


@pytest.fixture(scope="module")
def cond(golden, latents):
    g = golden("g7_frame_coarse")
    return g["signal"][0], g["signal_torso"].reshape(-1), latents[0][0], latents[1][0]


@pytest.fixture(scope="module")
def pix(scene):
    n = scene["H"] * scene["W"]
    idx = np.arange(11, n, n // N_RAYS)[:N_RAYS].astype(np.int32)          # a stride through the whole frame
    assert len(idx) == N_RAYS and N_RAYS % 8 != 0 and N_RAYS % 4 != 0
    return idx


@pytest.fixture(scope="module")
def bg(scene):
    return (t(scene["bg"]).float() / 255.0).reshape(-1, 3).cuda()


def _frame(eng, scene, nc, nf, fields, n=N_RAYS, begin=0):
    return eng.make_frame(scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"], scene["poses"][FRAME], scene["pose_body"],
                          scene["near"], scene["far"], ray_begin=begin, ray_count=n, n_coarse=nc, n_fine=nf, fields=fields)


def _render(eng, pk, cnd, scene, bg, pix, nc, nf, fields, **kw):
    sa, stt, zs, za = cnd
    bias = pk.fold(sa, stt if fields == 2 else None, zs, za)
    return eng.render(pk, bias, _frame(eng, scene, nc, nf, fields, n=len(pix)), bg, pix_index=t(pix).cuda(), **kw)


@pytest.fixture(scope="module")
def oracle(scene, states, latents, golden, pix):
    """the CPU oracle on the 93 rays, computed once per (n_coarse, n_fine, fields): -> dict with z_all of its own row-H pipeline and
    a function rgb_at(z) = decoder + compositing at given depths"""
    gc = golden("g7_frame_coarse")
    P = O.params_to_torch(states["decoder"])
    zs, za = [t(v) for v in latents]
    o_h, d_h = O.get_rays(scene["H"], scene["W"], scene["focal"], scene["poses"][FRAME][:3, :4], scene["cx"], scene["cy"])
    o_t, d_t = O.get_rays(scene["H"], scene["W"], scene["focal"], scene["pose_body"][:3, :4], scene["cx"], scene["cy"])
    sel = t(pix).long()
    rays = [x.reshape(-1, 3)[sel] for x in (o_h, d_h, o_t, d_t)]
    bgr = (t(scene["bg"]).float() / 255.0).reshape(-1, 3)[sel]
    sig, sigt = [t(gc["signal"]), None], t(gc["signal_torso"])
    cache = {}

    def get(nc, nf, fields):
        if (nc, nf, fields) not in cache:
            with torch.no_grad():
                _, _, aux = O.render_rays_chunk(P, *rays, bgr, scene["near"], scene["far"], zs, za, sig, sigt, nc, nf, fields,
                                                return_aux=True)
            cache[(nc, nf, fields)] = aux
        return cache[(nc, nf, fields)]

    def rgb_at(z, fields):
        with torch.no_grad():
            return O.render_fixed_samples(P, *rays, bgr, t(z), zs, za, sig, sigt, fields)
    return get, rgb_at


def test_the_rays_of_these_tests_do_not_all_look_alike(oracle):
    """what the sampler is fed, checked with the oracle on the CPU so that the tests below exercise more than one inverse CDF.  Head
    image: the coarse weights peak in many different bins (15 at 32 samples, 24 at 64).  Two-field image: the synthetic torso is
    opaque everywhere (tests/test_gpu_aux.py), so every ray's weight sits at the front - but spread over at least four bins, and no
    two rays get the same fine depths."""
    get, _ = oracle
    for nc in (32, 64):
        for fields in (1, 2):
            aux = get(nc, 32, fields)
            w = (aux["w_com_coarse"] if fields == 2 else aux["w_head_coarse"]).numpy()
            assert w.shape == (N_RAYS, nc)
            inner = w[:, 1:-1]                                   # what sample_pdf sees
            assert ((inner > 1e-3).sum(1) >= 4).all(), (nc, fields)
            assert len(np.unique(aux["z_fine"].numpy(), axis=0)) == N_RAYS, (nc, fields)
            if fields == 1:
                assert len(np.unique(inner.argmax(1))) >= nc // 4, (nc, np.unique(inner.argmax(1)))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["f32", "f16"])
@pytest.mark.parametrize("fields", [1, 2])
@pytest.mark.parametrize("nc,nf", PAIRS)
def test_sampler_is_bit_exact_given_the_coarse_weights(eng, packed, cond, scene, bg, pix, tier, fields, nc, nf):
    """test_gpu_parity.test_hierarchical_sampler_is_bit_exact_given_the_coarse_weights at the new pairs: the fused sampler + rank
    merge against oracle sample_pdf(fixed_order=True) + torch.sort fed with the kernel's own coarse weights (a coarse-only launch
    at the same n_coarse: identical arithmetic, identical bits).  At 32 coarse samples the normaliser's upper lanes hold 0.f -
    exactly what oracle.wave_sum64 pads with."""
    out = _render(eng, packed[tier], cond, scene, bg, pix, nc, 0, fields, want_weights=True, want_z=True)
    w = (out[3] if fields == 2 else out[2]).cpu()
    z = out[-1].cpu()
    assert np.array_equal(z.numpy(), O.coarse_z(scene["near"], scene["far"], nc)[None].expand(N_RAYS, nc).numpy())
    z_all = _render(eng, packed[tier], cond, scene, bg, pix, nc, nf, fields, want_z=True)[-1].cpu()
    assert z_all.shape == (N_RAYS, nc + nf)
    z_mid = .5 * (z[..., 1:] + z[..., :-1])
    z_f = O.sample_pdf(z_mid, w[..., 1:-1], nf, det=True, fixed_order=True)
    want, _ = torch.sort(torch.cat([z, z_f], -1), -1)
    assert np.array_equal(z_all.numpy(), want.numpy()), float((z_all - want).abs().max())


# ---- 2, 3 ---------------------------------------------------------------------------------------------------------------------------
def _f32_gates(eng, pk, cond, scene, bg, pix, oracle, nc, nf, fields):
    get, rgb_at = oracle
    out = _render(eng, pk, cond, scene, bg, pix, nc, nf, fields, want_weights=True, want_z=True)
    rh, rc, wh, wc, z = [None if o is None else o.cpu().numpy() for o in out]
    near, far = np.float32(scene["near"]), np.float32(scene["far"])
    assert z.shape == (N_RAYS, nc + nf) and (np.diff(z, axis=1) >= 0).all()
    assert (z[:, 0] == near).all() and (z[:, -1] == far).all()
    dz = np.abs(z - get(nc, nf, fields)["z_all"].numpy()).max()
    dh = np.abs(wh.sum(1) - 1.0).max()
    oh, oc = rgb_at(z, fields)
    eh = np.abs(rh - oh.numpy()).max()
    print(f"{nc}+{nf}, fields={fields}: max |z - oracle z| {dz:.3e} (bin {(far - near) / (nc - 1):.3e}), |sum w_head - 1| {dh:.2e}, "
          f"|rgb_head - oracle| {eh:.2e}")
    assert dz <= (float(far) - float(near)) / (nc - 1) * 1.001
    np.testing.assert_allclose(wh.sum(1), 1.0, atol=2e-6)
    np.testing.assert_allclose(rh, oh.numpy(), atol=5e-5, rtol=0)
    if fields == 2:
        print(f"    |sum w_com - 1| {np.abs(wc.sum(1) - 1.0).max():.2e}, |rgb_com - oracle| {np.abs(rc - oc.numpy()).max():.2e}")
        np.testing.assert_allclose(wc.sum(1), 1.0, atol=2e-6)
        np.testing.assert_allclose(rc, oc.numpy(), atol=5e-5, rtol=0)
    else:
        assert rc is None and wc is None


@pytest.mark.parametrize("fields", [1, 2])
@pytest.mark.parametrize("nc,nf", PAIRS)
def test_render_f32_vs_oracle_at_the_kernels_depths(eng, packed, cond, scene, bg, pix, oracle, fields, nc, nf):
    _f32_gates(eng, packed["f32"], cond, scene, bg, pix, oracle, nc, nf, fields)


def test_render_f16x3_32_plus_64_two_fields_carries_the_f32_gates(eng, packed, cond, scene, bg, pix, oracle):
    _f32_gates(eng, packed["f16x3"], cond, scene, bg, pix, oracle, 32, 64, 2)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["f16", "bf16"])
def test_u8_epilogue_equals_to8b_of_the_float_render_32_plus_64(eng, packed, cond, scene, bg, tier):
    """(a contiguous ray range in the middle of the frame; bf16: the training tier's inference kernels share the template)"""
    sa, stt, zs, za = cond
    pk = packed[tier]
    bias = pk.fold(sa, stt, zs, za)
    fr = _frame(eng, scene, 32, 64, 2, n=N_RAYS, begin=(scene["H"] // 2) * scene["W"] + 17)
    f_h, f_c = eng.render(pk, bias, fr, bg)[:2]
    u_h, u_c = eng.render_u8(pk, bias, fr, bg)
    assert u_h.dtype == torch.uint8 and tuple(u_h.shape) == (N_RAYS, 3) and float(f_c.std()) > 0.01
    assert torch.equal(u_h, eng.to8b(f_h)) and torch.equal(u_c, eng.to8b(f_c))


@pytest.mark.parametrize("tier", ["f16", "f32"])
def test_native_128_wide_program_equals_the_padded_one_32_plus_64(eng, golden, scene, bg, pix, tier):
    """the narrow network of tests/test_gpu_narrow.py (hidden width 128, z_dim 64), every output bit for bit"""
    flat = eng.flatten_state(synth.synth_decoder_state(0, z_dim=64, hidden=128), "cuda")
    g3 = golden("g3_decoder")
    zs, za = synth.synth_latents(0, z_dim=64)
    cnd = (g3["sig_aud"][0], g3["sig_torso"][0], zs[0], za[0])
    outs = []
    for width in (128, 256):
        pk = eng.PackedDecoder(flat, tier, z_dim=64, width=width)
        assert pk.width == width
        outs.append(_render(eng, pk, cnd, scene, bg, pix, 32, 64, 2, want_weights=True, want_z=True))
    assert len(outs[0]) == 5 and float(outs[0][1].std()) > 0.01
    for k, (a, b) in enumerate(zip(*outs)):
        assert a.shape == b.shape and torch.isfinite(a).all() and torch.equal(a, b), (tier, k, float((a - b).abs().max()))


@pytest.mark.parametrize("tier", ["f16", "f32"])
def test_rays_launch_fed_the_frames_own_rays_equals_the_plain_launch_64_plus_32(eng, packed, cond, scene, bg, pix, tier):
    sa, stt, zs, za = cond
    pk = packed[tier]
    plain = _render(eng, pk, cond, scene, bg, pix, 64, 32, 2, want_weights=True, want_z=True)
    geo = (scene["H"], scene["W"], scene["focal"])
    sel = t(pix).long().cuda()
    o_h, d_h = eng.get_rays(*geo, scene["poses"][FRAME], scene["cx"], scene["cy"])
    o_t, d_t = eng.get_rays(*geo, scene["pose_body"], scene["cx"], scene["cy"])
    rays = eng.pack_rays(*[x.reshape(-1, 3)[sel].contiguous() for x in (o_h, d_h, o_t, d_t)])
    junk = np.full((4, 4), 7.5, np.float32)              # a rays launch ignores the frame's poses and intrinsics
    fr = eng.make_frame(3, 5, 1.0, -2.0, 9.0, junk, junk, scene["near"], scene["far"], ray_begin=11, ray_count=N_RAYS, n_coarse=64,
                        n_fine=32, fields=2)
    got = eng.render(pk, pk.fold(sa, stt, zs, za), fr, bg[sel].contiguous(), rays=rays, want_weights=True, want_z=True)
    assert len(got) == len(plain) == 5 and got[-1].shape == (N_RAYS, 96) and float(plain[1].std()) > 0.01
    for k, (a, b) in enumerate(zip(got, plain)):
        assert torch.equal(a, b), (tier, k, float((a - b).abs().max()))


@pytest.mark.parametrize("tier", ["f16", "f32"])
@pytest.mark.parametrize("fields", [1, 2])
def test_aux_launch_32_plus_32(eng, packed, cond, scene, bg, pix, tier, fields):
    """the aux kernel's RGB is the plain kernel's bit for bit; acc / depth against the plain launch's own weights and depths summed
    over FG (every sample but the background plane) in float64, at tests/test_gpu_aux.py's bound for that comparison: S 2^-23 and
    z_far S 2^-23"""
    pk = packed[tier]
    S = 64
    rh, rc, wh, wc, z = [None if o is None else o.cpu().numpy()
                         for o in _render(eng, pk, cond, scene, bg, pix, 32, 32, fields, want_weights=True, want_z=True)]
    ah_rgb, ac_rgb, ah, ac = [None if o is None else o.cpu().numpy() for o in _render(eng, pk, cond, scene, bg, pix, 32, 32, fields, want_aux=True)]
    assert np.array_equal(ah_rgb, rh) and np.isfinite(rh).all() and float(rh.std()) > 0.01
    assert np.array_equal(ac_rgb, rc) if fields == 2 else (ac_rgb is None and ac is None)
    z_far = float(np.float32(scene["far"]))
    assert z.shape == (N_RAYS, S)
    for a, w in ((ah, wh), (ac, wc)):
        if a is None:
            continue
        assert a.shape == (N_RAYS, 2) and a.dtype == np.float32
        w64, z64 = w[:, :S - 1].astype(np.float64), z[:, :S - 1].astype(np.float64)         # (concate_bg: the last sample is the plane)
        e_acc, e_dep = np.abs(a[:, 0] - w64.sum(1)).max(), np.abs(a[:, 1] - (w64 * z64).sum(1)).max()
        print(f"{tier}, fields={fields}: |acc - acc64| {e_acc:.2e}, |depth - depth64| {e_dep:.2e}")
        assert e_acc <= S * 2.0 ** -23 and e_dep <= z_far * S * 2.0 ** -23


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc,nf", [(32, 64), (64, 32)])
def test_recording_forward_equals_the_inference_kernel(eng, states, cond, scene, bg, pix, nc, nf):
    """test_gpu_train_hier.test_hierarchical_forward_equals_the_inference_kernel at the new pairs, by a direct call of
    dfn_train_fwd_hier (training.TrainBuffers stays at 64 coarse samples): images and merged depths bit for bit, the ranks a
    permutation with the coarse points at theirs, and every slot of the recorded arrays written."""
    from dfanerf._lib import check, lib
    dev = torch.device("cuda")
    sa, stt, zs, za = cond
    n, S = N_RAYS, nc + nf
    NP = n * S
    pk = eng.PackedDecoder(eng.flatten_state(states["decoder"], dev), "f32")
    bias = pk.fold(sa, stt, zs, za)
    nh = pk.bias_floats(0)
    rows = [check(lib.dfn_train_rows(f, 0), "dfn_train_rows") for f in (0, 1)]
    mrows = [check(lib.dfn_train_rows(f, 2), "dfn_train_rows") for f in (0, 1)]
    assert NP % 32 == 0
    act = [torch.full((NP // 32, rows[f], 32), float("nan"), dtype=torch.float32, device=dev) for f in (0, 1)]      # [tile][row][point]
    masks = [torch.zeros(NP // 32, mrows[f], 64, dtype=torch.int32, device=dev) for f in (0, 1)]
    samples = torch.full((n, S, 8), float("nan"), dtype=torch.float32, device=dev)
    rgb = torch.full((2, n, 3), float("nan"), dtype=torch.float32, device=dev)
    z_all = torch.full((n, S), float("nan"), dtype=torch.float32, device=dev)
    ranks = torch.full((n, S), 255, dtype=torch.uint8, device=dev)
    px = t(pix).cuda()
    fr = _frame(eng, scene, nc, nf, 2)
    p = lambda x: C.c_void_p(x.data_ptr())
    check(lib.dfn_train_fwd_hier(0, C.byref(fr), p(pk.packed[0]), p(pk.packed[1]), p(bias), C.c_void_p(bias.data_ptr() + 4 * nh),
                                 p(bg), None, p(px), p(rgb[0]), p(rgb[1]), p(samples), p(act[0]), p(masks[0]), p(act[1]), p(masks[1]),
                                 p(z_all), p(ranks), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dfn_train_fwd_hier")
    rh, rc, z = eng.render(pk, bias, fr, bg, pix_index=px, want_z=True)
    torch.cuda.synchronize()
    assert torch.equal(rgb[0], rh) and torch.equal(rgb[1], rc) and torch.equal(z_all, z)
    rk = ranks.long().cpu()
    assert bool((torch.sort(rk, 1).values == torch.arange(S)[None]).all())                   # a permutation per ray
    zc = O.coarse_z(scene["near"], scene["far"], nc)
    assert torch.equal(torch.gather(z_all.cpu(), 1, rk[:, :nc]), zc[None].expand(n, nc))     # coarse points sit at their ranks
    # the fine points, in evaluation order, are the merged depths that are not coarse ones, ascending
    zf = torch.gather(z_all.cpu(), 1, rk[:, nc:])
    assert bool((zf[:, 1:] >= zf[:, :-1]).all())
    # every evaluated point was recorded: the raw outputs of both fields, and in every 32-point tile (the coarse tiles, then the
    # fine ones) the rows of every layer input the range guard reads (f16guard._groups)
    from dfanerf import f16guard
    assert bool(torch.isfinite(samples).all())
    for f in (0, 1):
        for name, a, b in f16guard._groups(f):
            assert bool(torch.isfinite(act[f][:, a:b, :]).all()), (f, name)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
def test_both_f16_guards_calibrate_at_32_plus_64(states, scene, latents, monkeypatch):
    from dfanerf import f16guard, run_nerf
    from dfanerf.decoder import Decoder
    dev = torch.device("cuda")
    dec = Decoder(z_dim=256, hidden_size=256, dim_signal=96, use_deformation_field=True)
    dec.load_state_dict({k: t(v) for k, v in states["decoder"].items()})
    dec.to(dev)
    args = run_nerf.config_parser().parse_args(
        "--expname t --concate_bg --dim_signal=96 --n_object=1 --use_deformation_field --render_person --hierarchical --N_samples 32 "
        "--N_importance 64 --hip_tier f16".split())
    run_nerf.check_supported(args)
    zs, za = [t(v).to(dev) for v in latents]
    plate = (t(scene["bg"]).float() / 255.0).to(dev)
    R = run_nerf.FrameRenderer(dec, zs, za, plate, [scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"]], scene["near"],
                               scene["far"], args)
    sh = t(synth.synth_tensor(0, "g3/sig", (96,), 0.8)).to(dev)
    st = t(synth.synth_tensor(0, "g3/sigt", (42,), 0.8)).to(dev)
    seen = []
    real = f16guard.activation_bounds

    def spy(flat, frames, *a, **kw):
        seen.append((int(frames[0].n_coarse), int(kw.get("n_fine", 0))))
        return real(flat, frames, *a, **kw)
    monkeypatch.setattr(f16guard, "activation_bounds", spy)
    assert R.check_f16(list(scene["poses"][:4]), scene["pose_body"], lambda k: (sh, st)) == "f16" and R.tier == "f16"
    assert seen == [(32, 64)]                                   # the range guard's calibration ran at the production counts
    pk = R.decoder.packed("f16")
    top = max(v for d in pk.f16_bounds.values() for v in d.values())
    assert 2.0 < top < 200.0 and set(pk.f16_accuracy) == {"head", "com"}
    gate = f16guard.psnr_gate(30.0)
    assert all(s["psnr_db"] >= gate and s["n_rays"] == 256 * 4 for s in pk.f16_accuracy.values()), pk.f16_accuracy
    # ... and the frame renders at those counts
    rh, rc = R.render(scene["poses"][0], scene["pose_body"], [sh[None], None], st, ray_begin=100000, ray_count=N_RAYS)
    assert torch.isfinite(rh).all() and torch.isfinite(rc).all() and float(rc.std()) > 0.01


def test_render_person_cli_32_plus_64_f16(dataset):
    from PIL import Image
    root, sc = dataset
    out = root / "dataset" / "train_together" / "obama_TrainExpLater_smoMix" / "obama" / "person"
    log = _run(root, "--render_person --test_file transforms_val_ba.json --N_rand=2048 --N_iters=600000 --image_ext png "
                     "--hierarchical --N_samples 32 --N_importance 64 --hip_tier f16")
    assert "f16 tier: calibrated on" in log
    for sub in ("render_com", "render_head"):
        assert sorted(os.listdir(out / sub)) == [f"test_{i:06d}.png" for i in range(F_VAL)]
        img = np.asarray(Image.open(out / sub / "test_000001.png").convert("RGB"))
        assert img.shape == (H, W, 3) and float(img.std()) > 2.55


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc,nf", [(32, 128), (64, 96), (128, 64), (48, 0)])
def test_refused_pairs_launch_nothing(eng, packed, cond, scene, bg, pix, nc, nf):
    from dfanerf._lib import DfnError
    sa, stt, zs, za = cond
    pk = packed["f32"]
    bias = pk.fold(sa, stt, zs, za)
    oh = torch.full((N_RAYS, 3), -7.0, device="cuda")
    oc = torch.full((N_RAYS, 3), -7.0, device="cuda")
    with pytest.raises(DfnError, match="n_coarse|n_fine"):
        eng.render(pk, bias, _frame(eng, scene, nc, nf, 2), bg, pix_index=t(pix).cuda(), out_head=oh, out_com=oc)
    torch.cuda.synchronize()
    assert bool((oh == -7.0).all()) and bool((oc == -7.0).all())


def test_training_at_32_plus_64_is_refused(scene):
    """the hierarchical step is 64 + 64 | 128: TrainBuffers refuses the pair, and so does the backward entry point - its output
    stays untouched"""
    from dfanerf import engine, training
    from dfanerf._lib import lib
    dev = torch.device("cuda")
    with pytest.raises(ValueError, match="TrainBuffers"):
        training.TrainBuffers("f32", 64, dev, n_fine=64, n_coarse=32)
    n, S = 64, 96
    fr = engine.make_frame(scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"], scene["poses"][1], scene["pose_body"], 0.3,
                           0.9, 1e10, 0, n, 32, 64, 2, True)
    samples = torch.zeros(n, S, 8, device=dev)
    z = torch.linspace(0.3, 0.9, S, device=dev)[None].repeat(n, 1).contiguous()
    ranks = torch.arange(S, dtype=torch.uint8, device=dev)[None].repeat(n, 1).contiguous()
    d = torch.ones(n, 3, device=dev)
    ds = torch.full((n, S, 8), -7.0, device=dev)
    pixi = torch.arange(n, dtype=torch.int32, device=dev)
    plate = (t(scene["bg"]).float() / 255.0).reshape(-1, 3).to(dev)
    p = lambda x: C.c_void_p(x.data_ptr())
    rc = lib.dfn_composite_bwd_hier(C.byref(fr), p(pixi), p(plate), None, p(samples), p(z), p(ranks), p(d), p(d), p(ds),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1 and b"64 coarse + 64 or 128 fine" in lib.dfn_last_error()
    torch.cuda.synchronize()
    assert bool((ds == -7.0).all())
