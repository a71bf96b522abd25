"""The fused renderer on caller-supplied rays (dfn_render_rays_fwd / dfn_render_rays_fwd_u8; csrc/dfn_render_*_rays.hip) on the GPU.
Rays come as data - f32 [R, 6 * fields] = o_head, d_head[, o_torso, d_torso], optional per-ray (near, far) - instead of being
generated from a pose and a pixel id; everything after the ray block of the kernel is the plain kernel's code.

  1. pinhole rays supplied = pinhole rays generated, bit for bit (every tier, sample count, field count, the u8 route, the 128-wide
     program; with and without bounds filled with the scene's near / far);
  2. rays of several cameras in one batch: each block equals the plain launch of its own pose, bit for bit;
  3. rays no pinhole makes (scaled directions, shifted origins, per-ray bounds; head and torso perturbed independently) against the
     CPU oracle at the project's f32 gates, in the f32 and the f16x3 tier;
  4. the f16 tier on the rays of 3.: PSNR against the oracle, gated 3 dB under the plain f16 kernel's on the unperturbed rays;
  5. refusals; 6. FrameRenderer.render_rays.

203 rays everywhere: whole workgroups plus a 3-ray tail at both 8 and 4 waves per workgroup."""
import ctypes as C

import numpy as np
import pytest
import torch

import dfa_oracle as O
from dfanerf import synth

pytestmark = pytest.mark.gpu

TIERS = ("f32", "f16", "f16x3")
FRAME = 2
R = 203
CONFIGS = [(64, 0, 2), (64, 128, 2), (64, 64, 2), (64, 128, 1), (32, 0, 2), (128, 0, 1)]      # (n_coarse, n_fine, fields)


def t(x):
    return torch.from_numpy(np.asarray(x))


def psnr(a, b):
    mse = float(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean())
    return 99.0 if mse == 0 else -10.0 * np.log10(mse)


@pytest.fixture(scope="module")
def eng():
    from dfanerf import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope="module")
def packed(eng, states):
    flat = eng.flatten_state(states["decoder"], "cuda")
    return {tier: eng.PackedDecoder(flat, tier) for tier in TIERS}


@pytest.fixture(scope="module")
def narrow(eng, golden):
    """a decoder of hidden width 128 on the native 128-wide program, as tests/test_gpu_narrow.py builds it"""
    flat = eng.flatten_state(synth.synth_decoder_state(0, z_dim=64, hidden=128), "cuda")
    g3 = golden("g3_decoder")
    zs, za = synth.synth_latents(0, z_dim=64)
    return ({tier: eng.PackedDecoder(flat, tier, z_dim=64, width=128) for tier in TIERS},
            (g3["sig_aud"][0], g3["sig_torso"][0], zs[0], za[0]))


@pytest.fixture(scope="module")
def cond(golden, latents):
    g = golden("g7_frame_coarse")
    return g["signal"][0], g["signal_torso"].reshape(-1), latents[0][0], latents[1][0]


@pytest.fixture(scope="module")
def pix(scene):
    n = scene["H"] * scene["W"]
    idx = np.arange(7, n, n // R)[:R].astype(np.int32)          # a stride through the frame
    assert len(idx) == R and R % 8 == 3 and R % 4 == 3
    return idx


@pytest.fixture(scope="module")
def bg(scene):
    return (t(scene["bg"]).float() / 255.0).reshape(-1, 3).cuda()


@pytest.fixture(scope="module")
def pinhole(eng, scene, pix):
    """k -> (o_head, d_head, o_torso, d_torso) [R,3] device tensors: engine.get_rays of poses[k] / pose_body at the pixels `pix`"""
    geo = (scene["H"], scene["W"], scene["focal"])
    sel = t(pix).long().cuda()
    cache = {}

    def get(k):
        if k not in cache:
            o_h, d_h = eng.get_rays(*geo, scene["poses"][k], scene["cx"], scene["cy"])
            o_t, d_t = eng.get_rays(*geo, scene["pose_body"], scene["cx"], scene["cy"])
            cache[k] = tuple(x.reshape(-1, 3)[sel].contiguous() for x in (o_h, d_h, o_t, d_t))
        return cache[k]
    return get


def _frame(eng, scene, n_coarse, n_fine, fields, frame_i=FRAME, n=R):
    return eng.make_frame(scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"], scene["poses"][frame_i], scene["pose_body"],
                          scene["near"], scene["far"], ray_count=n, n_coarse=n_coarse, n_fine=n_fine, fields=fields)


def _rays_frame(eng, scene, n_coarse, n_fine, fields, n=R):
    """the frame of a rays launch: the sample counts and near / far; poses and intrinsics are ignored - filled with junk on purpose"""
    junk = np.full((4, 4), 7.5, np.float32)
    return eng.make_frame(3, 5, 1.0, -2.0, 9.0, junk, junk, scene["near"], scene["far"], ray_begin=11, ray_count=n, n_coarse=n_coarse,
                          n_fine=n_fine, fields=fields)


def _pack(eng, r4, fields):
    return eng.pack_rays(r4[0], r4[1], *(r4[2:] if fields == 2 else ()))


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (what, i)
        if x is not None:
            assert x.shape == y.shape and torch.equal(x, y), (what, i, float((x.float() - y.float()).abs().max()))


def _plain_vs_rays(eng, pk, cnd, scene, bg, pix, r4, n_coarse, n_fine, fields, what):
    sa, stt, zs, za = cnd
    bias = pk.fold(sa, stt if fields == 2 else None, zs, za)
    px = t(pix).cuda()
    plain = eng.render(pk, bias, _frame(eng, scene, n_coarse, n_fine, fields), bg, pix_index=px, want_weights=True, want_z=True)
    assert torch.isfinite(plain[0]).all() and float(plain[0].std()) > 0.01, what
    assert plain[-1].shape == (R, n_coarse + n_fine)
    fr = _rays_frame(eng, scene, n_coarse, n_fine, fields)
    rays, bgr = _pack(eng, r4, fields), bg[px.long()].contiguous()
    got = eng.render(pk, bias, fr, bgr, rays=rays, want_weights=True, want_z=True)
    _same(got, plain, (what, "no bounds"))
    bounds = torch.tensor([scene["near"], scene["far"]], dtype=torch.float32).repeat(R, 1).cuda()
    got = eng.render(pk, bias, fr, bgr, rays=rays, bounds=bounds, want_weights=True, want_z=True)
    _same(got, plain, (what, "bounds = (near, far)"))
    # a uint8 background, one row per ray
    bg8 = t(scene["bg"]).reshape(-1, 3).cuda()
    plain8 = eng.render(pk, bias, _frame(eng, scene, n_coarse, n_fine, fields), bg8, pix_index=px)
    _same(eng.render(pk, bias, fr, bg8[px.long()].contiguous(), rays=rays), plain8, (what, "uint8 background"))


# ---- 1. pinhole rays supplied = pinhole rays generated ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_coarse,n_fine,fields", CONFIGS)
@pytest.mark.parametrize("tier", TIERS)
def test_supplied_pinhole_rays_equal_generated_rays_bitwise(eng, packed, cond, scene, bg, pix, pinhole, tier, n_coarse, n_fine, fields):
    _plain_vs_rays(eng, packed[tier], cond, scene, bg, pix, pinhole(FRAME), n_coarse, n_fine, fields, (tier, n_coarse, n_fine, fields))


@pytest.mark.parametrize("tier", TIERS)
def test_supplied_pinhole_rays_u8_route_bitwise(eng, packed, cond, scene, bg, pix, pinhole, tier):
    sa, stt, zs, za = cond
    pk = packed[tier]
    bias = pk.fold(sa, stt, zs, za)
    px = t(pix).cuda()
    plain = eng.render_u8(pk, bias, _frame(eng, scene, 64, 128, 2), bg, pix_index=px)
    assert plain[0].dtype == torch.uint8 and float(plain[1].float().std()) > 1.0
    rays, bgr = _pack(eng, pinhole(FRAME), 2), bg[px.long()].contiguous()
    fr = _rays_frame(eng, scene, 64, 128, 2)
    _same(eng.render_u8(pk, bias, fr, bgr, rays=rays), plain, (tier, "u8"))
    bounds = torch.tensor([scene["near"], scene["far"]], dtype=torch.float32).repeat(R, 1).cuda()
    oh, oc = torch.zeros(R, 3, dtype=torch.uint8, device="cuda"), torch.zeros(R, 3, dtype=torch.uint8, device="cuda")
    eng.render_u8(pk, bias, fr, bgr, rays=rays, bounds=bounds, out_head=oh, out_com=oc)
    _same((oh, oc), plain, (tier, "u8, bounds, caller's buffers"))


@pytest.mark.parametrize("tier", TIERS)
def test_supplied_pinhole_rays_width_128_bitwise(eng, narrow, scene, bg, pix, pinhole, tier):
    npk, ncond = narrow
    assert npk[tier].width == 128
    _plain_vs_rays(eng, npk[tier], ncond, scene, bg, pix, pinhole(FRAME), 64, 128, 2, (tier, "width 128"))


# ---- 2. several cameras in one batch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["f32", "f16"])
def test_rays_of_several_cameras_in_one_batch_bitwise(eng, packed, cond, scene, bg, pix, pinhole, tier):
    """per-ray state really is per ray: 70 + 70 + 63 rays of three poses in one launch, each block = the plain launch of its pose"""
    sa, stt, zs, za = cond
    pk = packed[tier]
    bias = pk.fold(sa, stt, zs, za)
    blocks = [(0, slice(0, 70)), (FRAME, slice(70, 140)), (5, slice(140, R))]
    rays = torch.cat([_pack(eng, pinhole(k), 2)[sl] for k, sl in blocks], 0)
    assert rays.shape == (R, 12) and not torch.equal(rays[0, :6], rays[70, :6])
    px = t(pix).cuda()
    got = eng.render(pk, bias, _rays_frame(eng, scene, 64, 128, 2), bg[px.long()].contiguous(), rays=rays, want_weights=True, want_z=True)
    for k, sl in blocks:
        n = sl.stop - sl.start
        plain = eng.render(pk, bias, _frame(eng, scene, 64, 128, 2, frame_i=k, n=n), bg, pix_index=px[sl].contiguous(),
                           want_weights=True, want_z=True)
        _same([g[sl] for g in got], plain, (tier, "pose", k))
    assert not torch.equal(got[0][:63], got[0][140:])


# ---- 3. rays no pinhole makes, against the oracle ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd(scene, pix):
    """the pinhole rays of `pix` (oracle's get_rays: engine.get_rays bit for bit, test_get_rays_bitwise_full_frame), perturbed with
    a fixed seed, head and torso independently: directions scaled by [0.8, 1.25], origins shifted by <= 0.02 per axis; per-ray
    bounds near in [0.28, 0.34], far in [0.8, 0.95].  CPU float32 tensors; "plain": the unperturbed rays."""
    geo = (scene["H"], scene["W"], scene["focal"])
    o_h, d_h = O.get_rays(*geo, scene["poses"][FRAME][:3, :4], scene["cx"], scene["cy"])
    o_t, d_t = O.get_rays(*geo, scene["pose_body"][:3, :4], scene["cx"], scene["cy"])
    sel = t(pix).long()
    plain = [x.reshape(-1, 3)[sel].contiguous() for x in (o_h, d_h, o_t, d_t)]
    rng = np.random.RandomState(20261017)
    f32 = lambda a: t(a.astype(np.float32))
    out = []
    for o, d in (plain[:2], plain[2:]):
        out.append(o + f32(rng.uniform(-0.02, 0.02, (R, 3))))
        out.append(d * f32(rng.uniform(0.8, 1.25, (R, 1))))
    bounds = torch.cat([f32(rng.uniform(0.28, 0.34, (R, 1))), f32(rng.uniform(0.8, 0.95, (R, 1)))], 1).contiguous()
    return {"plain": plain, "rays": [x.contiguous() for x in out], "bounds": bounds}


@pytest.fixture(scope="module")
def oracle_in(states, latents, golden, scene, pix):
    g = golden("g7_frame_coarse")
    zs, za = latents
    bgr = (t(scene["bg"]).float() / 255.0).reshape(-1, 3)[t(pix).long()]
    return {"P": O.params_to_torch(states["decoder"]), "zs": t(zs), "za": t(za), "sig": [t(g["signal"]), None],
            "sigt": t(g["signal_torso"]).reshape(1, -1), "bg": bgr}


def _oracle_at(oi, r4, z, fields, want_w=False):
    """-> rgb_head, w_head, rgb_com, w_com of the oracle at the depths z [R,S] (O.render_fixed_samples; the weights, where asked for,
    from the two calls it is made of)"""
    with torch.no_grad():
        rh, rc = O.render_fixed_samples(oi["P"], *r4, oi["bg"], z, oi["zs"], oi["za"], oi["sig"], oi["sigt"], fields)
        if not want_w:
            return rh, None, rc, None
        s_h, f_h, s_t, f_t = O._eval_fields(oi["P"], *r4, z, oi["zs"], oi["za"], oi["sig"], oi["sigt"], fields)
        rh2, w_h, rc2, w_c = O.integrate_fields(z, r4[1], r4[3], s_h, f_h, s_t, f_t, oi["bg"])
    assert torch.equal(rh2, rh) and (rc is None or torch.equal(rc2, rc))
    return rh, w_h, rc, w_c


def _launch_odd(eng, pk, cond, scene, odd, n_coarse, n_fine, fields, **kw):
    sa, stt, zs, za = cond
    bias = pk.fold(sa, stt if fields == 2 else None, zs, za)
    rays = _pack(eng, odd["rays"], fields).cuda()
    bgr = (t(scene["bg"]).float() / 255.0).reshape(-1, 3)[t(kw.pop("pix")).long()].contiguous().cuda()
    out = eng.render(pk, bias, _rays_frame(eng, scene, n_coarse, n_fine, fields), bgr, rays=rays, bounds=odd["bounds"].cuda(), **kw)
    return [None if o is None else o.cpu() for o in out]


@pytest.mark.parametrize("n_coarse,fields", [(64, 2), (32, 1)])
@pytest.mark.parametrize("tier", ["f32", "f16x3"])
def test_odd_rays_coarse_vs_oracle(eng, packed, cond, scene, pix, odd, oracle_in, tier, n_coarse, fields):
    """z_vals bitwise against O.coarse_z of each ray's own (near, far); weights within 2e-6 and RGB within 2e-5 of the oracle at
    those depths (the project's f32 gates)"""
    rh, rc, wh, wc, z = _launch_odd(eng, packed[tier], cond, scene, odd, n_coarse, 0, fields, pix=pix, want_weights=True, want_z=True)
    want_z = torch.cat([O.coarse_z(float(nr), float(fa), n_coarse)[None] for nr, fa in odd["bounds"]], 0)
    assert torch.equal(z, want_z), float((z - want_z).abs().max())
    assert float(z[:, 0].std()) > 0.01 and float(z[:, -1].std()) > 0.01          # the bounds really are per ray
    orh, owh, orc, owc = _oracle_at(oracle_in, odd["rays"], z, fields, want_w=True)
    errs = {"w_head": float((wh - owh).abs().max()), "rgb_head": float((rh - orh).abs().max())}
    if fields == 2:
        errs.update(w_com=float((wc - owc).abs().max()), rgb_com=float((rc - orc).abs().max()))
    print(f"{tier} coarse {n_coarse} x {fields}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + " (gates: w 2e-6, rgb 2e-5)")
    assert float(rh.std()) > 0.01 and (rc is None) == (fields == 1)
    for k, v in errs.items():
        assert v <= (2e-6 if k.startswith("w_") else 2e-5), (k, v)


@pytest.mark.parametrize("n_fine,fields", [(128, 2), (64, 1)])
@pytest.mark.parametrize("tier", ["f32", "f16x3"])
def test_odd_rays_hierarchical_vs_oracle(eng, packed, cond, scene, pix, odd, oracle_in, tier, n_fine, fields):
    """the merged depths bit-equal to sort(cat(z, sample_pdf(z_mid, w[1:-1]))) fed with the kernel's own coarse weights from the
    coarse-only rays launch (the construction of test_hierarchical_sampler_is_bit_exact_given_the_coarse_weights); RGB within
    5e-5 of the oracle at the kernel's depths"""
    co = _launch_odd(eng, packed[tier], cond, scene, odd, 64, 0, fields, pix=pix, want_weights=True, want_z=True)
    w, z = (co[3] if fields == 2 else co[2]), co[-1]
    rh, rc, z_all = _launch_odd(eng, packed[tier], cond, scene, odd, 64, n_fine, fields, pix=pix, want_z=True)
    z_mid = .5 * (z[..., 1:] + z[..., :-1])
    z_f = O.sample_pdf(z_mid, w[..., 1:-1], n_fine, det=True, fixed_order=True)
    want, _ = torch.sort(torch.cat([z, z_f], -1), -1)
    assert torch.equal(z_all, want), float((z_all - want).abs().max())
    orh, _, orc, _ = _oracle_at(oracle_in, odd["rays"], z_all, fields)
    errs = {"rgb_head": float((rh - orh).abs().max())}
    if fields == 2:
        errs["rgb_com"] = float((rc - orc).abs().max())
    print(f"{tier} 64 + {n_fine} x {fields}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + " (gate 5e-5)")
    for k, v in errs.items():
        assert v <= 5e-5, (k, v)


# ---- 4. the f16 tier on the rays of 3. ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fine", [0, 128])
def test_odd_rays_f16_psnr_vs_oracle(eng, packed, cond, scene, bg, pix, odd, oracle_in, n_fine):
    """PSNR of the f16 rays launch (perturbed rays, per-ray bounds; head and composite image together) against the oracle at the
    f32 rays launch's depths, gated 3 dB (f16guard's worst-frame allowance) under what the PLAIN f16 kernel scores against the
    oracle on the unperturbed rays of the same pixels, at the plain f32 launch's depths.
    Measured on an MI355X (printed on every run): 64 + 0: plain 71.58 dB, rays 72.20 dB (gate 68.58); 64 + 128: plain 67.12 dB,
    rays 67.33 dB (gate 64.12)."""
    sa, stt, zs, za = cond
    px = t(pix).cuda()
    score = {}
    # the baseline: the plain kernels, generated rays
    fr = _frame(eng, scene, 64, n_fine, 2)
    z32 = eng.render(packed["f32"], packed["f32"].fold(sa, stt, zs, za), fr, bg, pix_index=px, want_z=True)[-1].cpu()
    h16, c16 = [o.cpu() for o in eng.render(packed["f16"], packed["f16"].fold(sa, stt, zs, za), fr, bg, pix_index=px)]
    orh, _, orc, _ = _oracle_at(oracle_in, odd["plain"], z32, 2)
    score["plain"] = psnr(torch.cat([h16, c16]).numpy(), torch.cat([orh, orc]).numpy())
    # the code under test: supplied rays
    z32 = _launch_odd(eng, packed["f32"], cond, scene, odd, 64, n_fine, 2, pix=pix, want_z=True)[-1]
    h16, c16 = _launch_odd(eng, packed["f16"], cond, scene, odd, 64, n_fine, 2, pix=pix)
    orh, _, orc, _ = _oracle_at(oracle_in, odd["rays"], z32, 2)
    score["rays"] = psnr(torch.cat([h16, c16]).numpy(), torch.cat([orh, orc]).numpy())
    print(f"f16 64 + {n_fine}: plain kernel on the pinhole rays {score['plain']:.2f} dB, rays kernel on the perturbed rays "
          f"{score['rays']:.2f} dB (gate {score['plain'] - 3.0:.2f} dB)")
    assert score["rays"] >= score["plain"] - 3.0, score


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(eng, packed, states, cond, scene, bg, pix, pinhole):
    from dfanerf import _lib
    sa, stt, zs, za = cond
    pk = packed["f32"]
    bias = pk.fold(sa, stt, zs, za)
    px = t(pix).cuda()
    rays, bgr = _pack(eng, pinhole(FRAME), 2), bg[px.long()].contiguous()
    fr = _rays_frame(eng, scene, 64, 0, 2)
    oh, oc = torch.full((R, 3), -1.0, device="cuda"), torch.full((R, 3), -1.0, device="cuda")
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    nh = pk.bias_floats(0)
    common = (C.byref(fr), p(pk.packed[0]), p(pk.packed[1]), p(bias), C.c_void_p(bias.data_ptr() + 4 * nh))
    outs = (p(oh), p(oc), None, None, None, None)
    # the C ABI: NULL rays, bf16
    assert _lib.lib.dfn_render_rays_fwd(pk.tier_arg, *common, None, None, p(bgr), None, *outs) == -1
    assert b"rays is NULL" in _lib.lib.dfn_last_error()
    assert _lib.lib.dfn_render_rays_fwd(_lib.TIER_BF16, *common, p(rays), None, p(bgr), None, *outs) == -1
    assert b"bf16" in _lib.lib.dfn_last_error()
    assert _lib.lib.dfn_render_rays_fwd_u8(_lib.TIER_BF16, *common, p(rays), None, p(bgr), None, p(oh), p(oc), None) == -1
    # ... and through engine: a bf16 decoder
    pkb = eng.PackedDecoder(eng.flatten_state(states["decoder"], "cuda"), "bf16")
    with pytest.raises(Exception, match="bf16"):
        eng.render(pkb, pkb.fold(sa, stt, zs, za), fr, bgr, rays=rays, out_head=oh, out_com=oc)
    # rays together with what has no rays form
    for kw in ({"pix_index": px}, {"want_aux": True}):
        with pytest.raises(ValueError, match="rays cannot be combined with " + next(iter(kw))):
            eng.render(pk, bias, fr, bgr, rays=rays, out_head=oh, out_com=oc, **kw)
    for kw in ({"pix_index": px}, {"want_alpha": True}, {"want_depth": True}):
        with pytest.raises(ValueError, match="rays cannot be combined with " + next(iter(kw))):
            eng.render_u8(pk, bias, fr, bgr, rays=rays, **kw)
    # ray_count != rows, a background with the wrong row count (the whole plate), rows of the wrong width
    with pytest.raises(ValueError, match="ray_count"):
        eng.render(pk, bias, _rays_frame(eng, scene, 64, 0, 2, n=R - 1), bgr[:R - 1].contiguous(), rays=rays, out_head=oh, out_com=oc)
    with pytest.raises(ValueError, match="bg"):
        eng.render(pk, bias, fr, bg, rays=rays, out_head=oh, out_com=oc)
    with pytest.raises(ValueError, match="bg"):
        eng.render_u8(pk, bias, fr, bgr[:R - 1].contiguous(), rays=rays)
    with pytest.raises(ValueError, match="12"):
        eng.render(pk, bias, fr, bgr, rays=rays[:, :6].contiguous(), out_head=oh, out_com=oc)
    with pytest.raises(ValueError, match="bounds"):
        eng.render(pk, bias, fr, bgr, rays=rays, bounds=torch.zeros(R, 3, device="cuda"), out_head=oh, out_com=oc)
    with pytest.raises(ValueError, match="bounds"):
        eng.render(pk, bias, _frame(eng, scene, 64, 0, 2), bg, bounds=torch.zeros(R, 2, device="cuda"), out_head=oh, out_com=oc)
    # the hierarchical mode keeps its coarse sample count
    with pytest.raises(Exception, match="n_coarse = 64"):
        eng.render(pk, bias, _rays_frame(eng, scene, 32, 128, 2), bgr, rays=rays, out_head=oh, out_com=oc)
    torch.cuda.synchronize()
    assert float(oh.max()) == -1.0 and float(oc.max()) == -1.0             # none of the refused calls wrote anything


# ---- 6. FrameRenderer.render_rays ------------------------------------------------------------------------------------------------------
def test_frame_renderer_render_rays_equals_render(eng, scene, golden, bg, pix, pinhole):
    from dfanerf import run_nerf
    from dfanerf.decoder import Decoder
    dev = torch.device("cuda")
    g3 = golden("g3_decoder")
    dec = Decoder(z_dim=64, hidden_size=256, dim_signal=96, use_deformation_field=True)
    dec.load_state_dict({k: t(v) for k, v in synth.synth_decoder_state(0, z_dim=64).items()})
    dec.to(dev)
    zs, za = [t(v).to(dev) for v in synth.synth_latents(0, z_dim=64)]
    sa, stt = t(g3["sig_aud"]).to(dev), t(g3["sig_torso"]).to(dev)
    args = run_nerf.config_parser().parse_args("--expname t --concate_bg --dim_signal=96 --n_object=1 --use_deformation_field --z_dim 64 "
                                               "--render_person --hierarchical --N_importance 128 --hip_tier f16".split())
    run_nerf.check_supported(args)
    plate = (t(scene["bg"]).float() / 255.0).to(dev)
    FR = run_nerf.FrameRenderer(dec, zs, za, plate, [scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"]], scene["near"],
                                scene["far"], args)
    px = t(pix).cuda()
    o_h, d_h, o_t, d_t = pinhole(FRAME)
    for fields in (2, 1):
        want = FR.render(scene["poses"][FRAME], scene["pose_body"], [sa, None], stt[0], pix_index=px, fields=fields, out_u8=True)
        got = FR.render_rays((o_h, d_h), (o_t, d_t) if fields == 2 else None, [sa, None], stt[0], bg[px.long()], fields=fields, out_u8=True)
        assert want[0].dtype == torch.uint8 and float(want[0].float().std()) > 1.0
        _same(got, want, ("FrameRenderer u8", fields))
    # the float route, per-ray bounds equal to the renderer's near / far, the caller's buffers
    want = FR.render(scene["poses"][FRAME], scene["pose_body"], [sa, None], stt[0], pix_index=px)
    out = (torch.zeros(R, 3, device=dev), torch.zeros(R, 3, device=dev))
    bounds = torch.tensor([scene["near"], scene["far"]], dtype=torch.float32).repeat(R, 1)
    FR.render_rays((o_h, d_h), (o_t, d_t), [sa, None], stt[0], bg[px.long()], bounds=bounds, out=out)
    _same(out, want, "FrameRenderer f32")
