"""The 128-wide inference program on the GPU (DFN_WIDTH_128; csrc/dfn_render_*_w128.hip): for a network of hidden width <= 128 it
must return THE SAME BITS as the padded 256-wide program - zero padding contributes exact zero products, the dropped MFMAs are the
all-zero trailing k-units of each activation segment, the dropped output tiles feed zero columns only, and the accumulation order of
the surviving terms is unchanged in all three tiers.  Network: golden G18's, the reference's Decoder(hidden_size=128, z_dim=64)."""
import numpy as np
import pytest
import torch

from dfanerf import synth

pytestmark = pytest.mark.gpu

TIERS = ("f32", "f16", "f16x3")
N_RAYS = 1003            # a ragged last workgroup in every tier (8 and 4 rays per workgroup)
t = torch.from_numpy


@pytest.fixture(scope="module")
def eng():
    from dfanerf import engine
    engine.require_gpu()
    return engine


def _pair(eng, tier, hidden=128, z_dim=64):
    """the same flat parameter vector packed for the native 128-wide program and for the padded one"""
    flat = eng.flatten_state(synth.synth_decoder_state(0, z_dim=z_dim, hidden=hidden), "cuda")
    return (eng.PackedDecoder(flat, tier, fields=(0, 1, 2), z_dim=z_dim, width=128),
            eng.PackedDecoder(flat, tier, fields=(0, 1, 2), z_dim=z_dim, width=256))


@pytest.fixture(scope="module")
def packs(eng):
    return {tier: _pair(eng, tier) for tier in TIERS}


@pytest.fixture(scope="module")
def cond(golden):
    g3 = golden("g3_decoder")
    zs, za = synth.synth_latents(0, z_dim=64)
    return g3["sig_aud"][0], g3["sig_torso"][0], zs[0], za[0]


def _render(eng, pk, scene, cond, fields, n_coarse, n_fine, u8=False, frame=1, begin=None):
    sa, stt, zs, za = cond
    bias = pk.fold(sa, stt if fields == 2 else None, zs, za)
    begin = (scene["H"] // 2) * scene["W"] + 17 if begin is None else begin          # the middle of the frame
    fr = eng.make_frame(scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"], scene["poses"][frame], scene["pose_body"],
                        scene["near"], scene["far"], ray_begin=begin, ray_count=N_RAYS, n_coarse=n_coarse, n_fine=n_fine,
                        fields=fields)
    bg = (t(scene["bg"]).float() / 255.0).reshape(-1, 3).cuda()
    if u8:
        out = eng.render_u8(pk, bias, fr, bg)
    else:
        out = eng.render(pk, bias, fr, bg, want_weights=True, want_z=True)
    torch.cuda.synchronize()
    return [o for o in out if o is not None]


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and bool(torch.isfinite(x.float()).all()), (what, k)
        if not torch.equal(x, y):
            d = (x.float() - y.float()).abs()
            raise AssertionError(f"{what}: output {k} differs in {int((d > 0).sum())} of {d.numel()} values, max |diff| {float(d.max()):.3e}")


@pytest.mark.parametrize("tier", TIERS)
def test_bitwise_against_the_padded_program_hierarchical(eng, packs, scene, cond, tier):
    n, w = packs[tier]
    assert n.width == 128 and w.width == 256 and n.packed[0].numel() < w.packed[0].numel()
    a, b = (_render(eng, pk, scene, cond, 2, 64, 128) for pk in (n, w))
    assert len(a) == 5                                   # rgb head / composite, both weight arrays, depths
    _same(a, b, f"{tier}, two fields, 64 + 128")
    assert float(a[0].std()) > 0.01 and float(a[1].std()) > 0.01      # not an all-background patch


@pytest.mark.parametrize("tier", TIERS)
def test_bitwise_head_only_and_coarse_only(eng, packs, scene, cond, tier):
    n, w = packs[tier]
    a, b = (_render(eng, pk, scene, cond, 1, 64, 128) for pk in (n, w))
    _same(a, b, f"{tier}, head only, 64 + 128")
    assert float(a[0].std()) > 0.01
    a, b = (_render(eng, pk, scene, cond, 2, 32, 0) for pk in (n, w))
    _same(a, b, f"{tier}, two fields, 32 coarse")
    assert float(a[0].std()) > 0.01 and float(a[1].std()) > 0.01


@pytest.mark.parametrize("tier", TIERS)
def test_bitwise_u8_epilogue(eng, packs, scene, cond, tier):
    n, w = packs[tier]
    a, b = (_render(eng, pk, scene, cond, 2, 64, 128, u8=True) for pk in (n, w))
    assert a[0].dtype == torch.uint8 and len(a) == 2
    _same(a, b, f"{tier}, uint8 epilogue")
    assert float(a[1].float().std()) > 2.55


@pytest.mark.parametrize("tier", TIERS)
def test_bitwise_decoder_forward(eng, packs, golden, cond, tier):
    n, w = packs[tier]
    g3 = golden("g3_decoder")
    sa, stt, zs, za = cond
    p, r = g3["p_64"].reshape(-1, 3), g3["r_64"].reshape(-1, 3)          # 4 x 64 points
    for field, sig, row in ((0, sa, 0), (1, stt, 1), (2, None, 0)):
        out = []
        for pk in (n, w):
            bias = pk.fold_single(field, sig, zs[row], za[row])
            out.append(eng.decoder_forward(pk, field, bias, p, r))
        torch.cuda.synchronize()
        _same(out[0], out[1], f"{tier}, decoder_forward field {field}")
        assert float(out[0][0].std()) > 1e-3


def test_native_program_meets_the_reference_golden(golden):
    """test_gpu_parity.test_narrower_decoder_vs_reference_golden's gates, through the native program"""
    from dfanerf.decoder import Decoder
    dev = torch.device("cuda")
    g, g3 = golden("g18_n_feat_128"), golden("g3_decoder")
    dec = Decoder(z_dim=64, hidden_size=128, dim_signal=96, use_deformation_field=True)
    dec.load_state_dict({k: t(v) for k, v in synth.synth_decoder_state(0, z_dim=64, hidden=128).items()})
    dec.to(dev)
    assert dec.packed("f32").width == 128 and dec.packed("f16").width == 128 and dec.packed("bf16").width == 256
    zs, za = [t(v).to(dev) for v in synth.synth_latents(0, z_dim=64)]
    p, r = t(g3["p_64"]).to(dev), t(g3["r_64"]).to(dev)
    sa, stt = t(g3["sig_aud"]).to(dev), t(g3["sig_torso"]).to(dev)
    with torch.no_grad():
        out = {"head": dec(p, r, zs[:, 0], za[:, 0], [sa, None], "head"), "torso": dec(p, r, zs[:, 1], za[:, 1], stt, "torso"),
               "listener": dec(p, r, zs[:, 0], za[:, 0], [None, None], "head")}
    for k, (f, s) in out.items():
        np.testing.assert_allclose(f.cpu().numpy(), g["feat_" + k], atol=1e-5, rtol=0)
        np.testing.assert_allclose(s.cpu().numpy(), g["sigma_" + k], rtol=1e-5, atol=2e-4)
    with torch.no_grad():
        f16, _ = dec(p, r, zs[:, 1], za[:, 1], stt, "torso", tier="f16")
    assert float((f16.cpu() - t(g["feat_torso"])).abs().max()) < 3e-3


@pytest.mark.parametrize("tier", TIERS)
def test_bitwise_narrower_than_128(eng, scene, golden, tier):
    """hidden 64, z_dim 32: zero tiles INSIDE the narrow program"""
    g3 = golden("g3_decoder")
    n, w = _pair(eng, tier, hidden=64, z_dim=32)
    zs, za = synth.synth_latents(0, z_dim=32)
    cond = (g3["sig_aud"][0], g3["sig_torso"][0], zs[0], za[0])
    a, b = (_render(eng, pk, scene, cond, 2, 64, 128) for pk in (n, w))
    _same(a, b, f"{tier}, hidden 64")
    assert float(a[0].std()) > 0.01 and float(a[1].std()) > 0.01


def test_frame_renderer_f16x3_range_guard_and_width_switch(scene, golden, monkeypatch):
    """FrameRenderer gets the narrow program through Decoder.packed: --hip_tier f16x3 --hierarchical on the 128-wide decoder passes
    its range guard, and the frame equals the one rendered with DFN_WIDTH=256 (the A/B switch, read when the pack is built)"""
    from dfanerf import run_nerf
    from dfanerf.decoder import Decoder
    dev = torch.device("cuda")
    g3 = golden("g3_decoder")
    monkeypatch.delenv("DFN_WIDTH", raising=False)
    args = run_nerf.config_parser().parse_args("--expname t --concate_bg --dim_signal=96 --n_object=1 --use_deformation_field --z_dim 64 "
                                               "--n_feat 128 --render_person --hierarchical --N_importance 128 --hip_tier f16x3".split())
    run_nerf.check_supported(args)
    zs, za = [t(v).to(dev) for v in synth.synth_latents(0, z_dim=64)]
    sa, stt = t(g3["sig_aud"]).to(dev), t(g3["sig_torso"]).to(dev)
    bg = (t(scene["bg"]).float() / 255.0).to(dev)
    geo = [scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"]]
    frames = []
    for force in (None, "256"):
        if force:
            monkeypatch.setenv("DFN_WIDTH", force)
        dec = Decoder(z_dim=64, hidden_size=128, dim_signal=96, use_deformation_field=True)
        dec.load_state_dict({k: t(v) for k, v in synth.synth_decoder_state(0, z_dim=64, hidden=128).items()})
        dec.to(dev)
        R = run_nerf.FrameRenderer(dec, zs, za, bg, geo, scene["near"], scene["far"], args)
        assert R.tier == "f16x3" and dec.packed("f16x3").width == (256 if force else 128)
        bounds = R.check_f16_range(scene["poses"][:2], scene["pose_body"], lambda k: (sa[0], stt[0]), max_frames=2, n_rays=64)
        assert bounds and all(np.isfinite(v) for layers in bounds.values() for v in layers.values())
        frames.append(R.render(scene["poses"][1], scene["pose_body"], [sa, None], stt[0],
                               ray_begin=(scene["H"] // 2) * scene["W"], ray_count=N_RAYS))
    (a_h, a_c), (b_h, b_c) = frames
    assert torch.equal(a_h, b_h) and torch.equal(a_c, b_c) and float(a_c.std()) > 0.01
