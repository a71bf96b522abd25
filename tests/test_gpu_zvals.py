"""Rendering at caller-supplied depths (dfn_render_z_fwd / _u8), the stand-alone fine sampler (dfn_fine_depths) and the two-launch
hierarchical render built on them (engine.render_two_pass), on the GPU.

  1. a z launch fed the coarse depths of a plain coarse-only launch returns that launch's RGB, weights and depths bit for bit: tiers
     f32 / f16 / f16x3, one and two fields, 32 / 64 / 128 samples, both widths, the u8 form, with and without pix_index, 93 rays;
  2. the counts only a z launch has - 96, 160, 192 - at random sorted depths (repeated values, last depth = far) against the CPU
     oracle's render_fixed_samples: the project's equal-depth gates (RGB 5e-5, weight sums 2e-6) in the exact tiers, and on the blend
     decoder every single weight at tests/test_gpu_blend.py's gate (4 x blend_scene.W_F64, the reference's own f64-vs-f32 difference);
  3. dfn_fine_depths on a coarse launch's weights = the z_all of the hierarchical launch of the same tier, bit for bit, and = oracle
     sample_pdf(fixed_order=True) + sort on the same weights: five pairs, f32 and f16, one and two fields, both decoders;
  4. render_two_pass with ONE decoder for both passes = the one-launch hierarchical render: depths, RGB and the u8 form bit for bit.

93 rays (tests/blend_scene.py's stride through frame 2): no multiple of 4 or 8, the last workgroup has idle waves in every tier."""
import numpy as np
import pytest
import torch

import blend_scene as B
import dfa_oracle as O
from dfanerf import synth

pytestmark = pytest.mark.gpu

N_RAYS, FRAME = B.N_RAYS, B.FRAME
HIER_PAIRS = [(32, 32), (32, 64), (64, 32), (64, 64), (64, 128)]
W_GATE = {name: 4.0 * v for name, v in B.W_F64.items()}          # tests/test_gpu_blend.py's per-weight gate on the blend decoder
t = B.t


@pytest.fixture(scope="module")
def eng():
    from dfanerf import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope="module")
def dec_states(states):
    return {"fix": states["decoder"], "blend": B.blend_state(states)}


@pytest.fixture(scope="module")
def packed(eng, dec_states):
    cache = {}

    def get(scene_name, tier):
        if (scene_name, tier) not in cache:
            if scene_name not in cache:
                cache[scene_name] = eng.flatten_state(dec_states[scene_name], "cuda")
            cache[(scene_name, tier)] = eng.PackedDecoder(cache[scene_name], tier)
        return cache[(scene_name, tier)]
    return get


@pytest.fixture(scope="module")
def cond(golden, latents):
    return B.conditioning(golden("g7_frame_coarse"), latents)


@pytest.fixture(scope="module")
def pix(scene):
    idx = B.ray_indices(scene)
    assert len(idx) == N_RAYS and N_RAYS % 8 != 0 and N_RAYS % 4 != 0
    return idx


@pytest.fixture(scope="module")
def bg(scene):
    return (t(scene["bg"]).float() / 255.0).reshape(-1, 3).cuda()


@pytest.fixture(scope="module")
def orcs(scene, dec_states, latents, golden, pix):
    g7 = golden("g7_frame_coarse")
    return {k: B.Oracle(scene, v, latents, g7, pix) for k, v in dec_states.items()}


def _frame(eng, scene, nc, nf, fields, n=N_RAYS, begin=0):
    return eng.make_frame(scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"], scene["poses"][FRAME], scene["pose_body"],
                          scene["near"], scene["far"], ray_begin=begin, ray_count=n, n_coarse=nc, n_fine=nf, fields=fields)


def _bias(pk, cnd, fields):
    sa, stt, zs, za = cnd
    return pk.fold(sa, stt if fields == 2 else None, zs, za)


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        if b is None:
            assert a is None, (what, k)
        else:
            assert a.shape == b.shape and bool(torch.isfinite(b.float()).all()) and torch.equal(a, b), \
                (what, k, float((a.float() - b.float()).abs().max()))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
def _identity(eng, pk, cnd, scene, bg, pix, fields, what):
    bias = _bias(pk, cnd, fields)
    px = t(pix).cuda()
    begin = (scene["H"] // 2) * scene["W"] + 17
    for nc in (32, 64, 128):
        for kw, fr in (({"pix_index": px}, _frame(eng, scene, nc, 0, fields)), ({}, _frame(eng, scene, nc, 0, fields, begin=begin))):
            plain = eng.render(pk, bias, fr, bg, want_weights=True, want_z=True, **kw)
            z = plain[-1]
            assert z.shape == (N_RAYS, nc) and float(plain[0].std()) > 0.01
            got = eng.render(pk, bias, fr, bg, want_weights=True, want_z=True, z_vals=z.clone(), **kw)
            _same(got, plain, (what, nc, bool(kw)))
            _same(eng.render_u8(pk, bias, fr, bg, z_vals=z, **kw), eng.render_u8(pk, bias, fr, bg, **kw), (what, nc, bool(kw), "u8"))
    # the outputs are optional one by one, as in the plain call
    fr = _frame(eng, scene, 64, 0, fields)
    z = eng.render(pk, bias, fr, bg, pix_index=px, want_z=True)[-1]
    _same(eng.render(pk, bias, fr, bg, pix_index=px, z_vals=z), eng.render(pk, bias, fr, bg, pix_index=px), (what, "rgb only"))


@pytest.mark.parametrize("tier", ["f32", "f16", "f16x3"])
@pytest.mark.parametrize("fields", [1, 2])
def test_z_launch_fed_the_plain_launchs_depths_equals_it(eng, packed, cond, scene, bg, pix, tier, fields):
    _identity(eng, packed("blend" if fields == 2 else "fix", tier), cond, scene, bg, pix, fields, (tier, fields))


@pytest.mark.parametrize("tier", ["f32", "f16", "f16x3"])
def test_z_launch_equals_the_plain_launch_in_the_native_128_wide_program(eng, golden, scene, bg, pix, tier):
    """the narrow network of tests/test_gpu_narrow.py (hidden width 128, z_dim 64), two fields and one"""
    flat = eng.flatten_state(synth.synth_decoder_state(0, z_dim=64, hidden=128), "cuda")
    g3 = golden("g3_decoder")
    zs, za = synth.synth_latents(0, z_dim=64)
    cnd = (g3["sig_aud"][0], g3["sig_torso"][0], zs[0], za[0])
    pk = eng.PackedDecoder(flat, tier, z_dim=64, width=128)
    assert pk.width == 128
    for fields in (2, 1):
        _identity(eng, pk, cnd, scene, bg, pix, fields, (tier, "w128", fields))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
def _random_depths(scene, nc, seed):
    """sorted uniform depths in [near, far], different on every ray; repeated values (a pair and a triple per ray, on some rays the
    first two and the last two as well) and the last depth equal to far"""
    rng = np.random.RandomState(seed)
    near, far = np.float32(scene["near"]), np.float32(scene["far"])
    z = np.sort(rng.uniform(near, far, (N_RAYS, nc)).astype(np.float32), 1)
    z[:, -1] = far
    z[:, 10] = z[:, 9]
    z[:, nc // 2 + 1] = z[:, nc // 2 + 2] = z[:, nc // 2]
    z[::5, 0] = near
    z[::7, 1] = z[::7, 0]
    z[::3, -2] = far
    assert (np.diff(z, axis=1) >= 0).all() and (np.diff(z, axis=1) == 0).sum() >= 3 * N_RAYS
    return z


_ORACLE_AT = {}


def _oracle_at(orcs, name, scene, nc):
    """the oracle at the random depths of (decoder, count), computed once and shared by the tiers"""
    if (name, nc) not in _ORACLE_AT:
        z = _random_depths(scene, nc, nc)
        _ORACLE_AT[(name, nc)] = (z, [x.numpy() for x in orcs[name].at(z)])
    return _ORACLE_AT[(name, nc)]


@pytest.mark.parametrize("tier", ["f32", "f16x3"])
@pytest.mark.parametrize("nc", [96, 160, 192])
@pytest.mark.parametrize("name", ["fix", "blend"])
def test_new_counts_vs_oracle_at_random_depths(eng, packed, cond, scene, bg, pix, orcs, name, nc, tier):
    z, (oh, owh, oc, owc) = _oracle_at(orcs, name, scene, nc)
    pk = packed(name, tier)
    rh, rc, wh, wc, zo = [o.cpu().numpy() for o in eng.render(pk, _bias(pk, cond, 2), _frame(eng, scene, nc, 0, 2), bg,
                                                               pix_index=t(pix).cuda(), want_weights=True, want_z=True,
                                                               z_vals=t(z).cuda())]
    assert np.array_equal(zo, z)
    e = {"rgb_head": np.abs(rh - oh).max(), "rgb_com": np.abs(rc - oc).max(), "w_head": np.abs(wh - owh).max(),
         "w_com": np.abs(wc - owc).max(), "sum w_head": np.abs(wh.sum(1) - 1.0).max(), "sum w_com": np.abs(wc.sum(1) - 1.0).max()}
    print(f"{name} {tier} {nc} depths: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert float(oh.std()) > 0.01 and float(oc.std()) > 0.01
    np.testing.assert_allclose(wh.sum(1), 1.0, atol=2e-6)
    np.testing.assert_allclose(wc.sum(1), 1.0, atol=2e-6)
    np.testing.assert_allclose(rh, oh, atol=5e-5, rtol=0)
    np.testing.assert_allclose(rc, oc, atol=5e-5, rtol=0)
    # a zero-length interval carries no weight
    assert (wh[:, 9] == 0).all() and (wc[:, 9] == 0).all()
    if name == "blend":
        np.testing.assert_allclose(wh, owh, atol=W_GATE["head"], rtol=0)
        np.testing.assert_allclose(wc, owc, atol=W_GATE["com"], rtol=0)


def test_new_count_one_field_f32_vs_oracle(eng, packed, cond, scene, bg, pix, orcs):
    z = _random_depths(scene, 160, 7)
    oh, owh = [x.numpy() for x in orcs["blend"].at(z, fields=1)[:2]]
    pk = packed("blend", "f32")
    rh, rc, wh, wc = eng.render(pk, _bias(pk, cond, 1), _frame(eng, scene, 160, 0, 1), bg, pix_index=t(pix).cuda(), want_weights=True,
                                z_vals=t(z).cuda())
    assert rc is None and wc is None
    np.testing.assert_allclose(wh.cpu().numpy().sum(1), 1.0, atol=2e-6)
    np.testing.assert_allclose(rh.cpu().numpy(), oh, atol=5e-5, rtol=0)
    np.testing.assert_allclose(wh.cpu().numpy(), owh, atol=W_GATE["head"], rtol=0)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fix", "blend"])
@pytest.mark.parametrize("nc,nf", HIER_PAIRS)
def test_fine_depths_equals_the_fused_sampler_and_the_oracle(eng, packed, cond, scene, bg, pix, name, nc, nf):
    px = t(pix).cuda()
    for tier in ("f32", "f16"):
        pk = packed(name, tier)
        for fields in (1, 2):
            bias = _bias(pk, cond, fields)
            out = eng.render(pk, bias, _frame(eng, scene, nc, 0, fields), bg, pix_index=px, want_weights=True, want_z=True)
            w, z = (out[3] if fields == 2 else out[2]), out[-1].cpu()
            fr = _frame(eng, scene, nc, nf, fields)
            fused = eng.render(pk, bias, fr, bg, pix_index=px, want_z=True)[-1]
            twin = eng.fine_depths(fr, w)
            assert twin.shape == (N_RAYS, nc + nf) and torch.equal(twin, fused), (tier, fields, float((twin - fused).abs().max()))
            z_f = O.sample_pdf(.5 * (z[..., 1:] + z[..., :-1]), w.cpu()[..., 1:-1], nf, det=True, fixed_order=True)
            want, _ = torch.sort(torch.cat([z, z_f], -1), -1)
            assert np.array_equal(twin.cpu().numpy(), want.numpy()), (tier, fields, float((twin.cpu() - want).abs().max()))
            assert fields == 1 or len(np.unique(z_f.numpy(), axis=0)) == N_RAYS      # (not one inverse CDF)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", ["f32", "f16"])
@pytest.mark.parametrize("name", ["fix", "blend"])
def test_two_pass_with_one_tier_equals_the_one_launch_render(eng, packed, cond, scene, bg, pix, name, tier):
    """The same decoder in both passes against the one-launch hierarchical render: depths, images and the u8 form bit for bit.  Every
    point's decoder output is bit-identical (an MFMA column depends on its own point only: DESIGN.md 4), the fed-back depths are the
    fused sampler's, and a z launch composites the merged samples tile by tile in the fused kernel's order with the same f32
    arithmetic - so nothing may differ, in any tier."""
    px = t(pix).cuda()
    pk = packed(name, tier)
    for nc, nf in ((32, 32), (64, 128)):
        for fields in (2, 1):
            bias = _bias(pk, cond, fields)
            fr = _frame(eng, scene, nc, nf, fields)
            one = eng.render(pk, bias, fr, bg, pix_index=px, want_z=True)
            two = eng.render_two_pass(pk, bias, pk, bias, fr, bg, pix_index=px, want_z=True)
            assert torch.equal(two[2], one[2]), (nc, nf, fields)
            _same(two[:2], one[:2], (name, tier, nc, nf, fields))
            assert float(one[0].std()) > 0.01 and (fields == 2) == (two[1] is not None)
            ws = eng.two_pass_workspace(pk, fr)                    # the caller's buffers: the same launches, the same bits
            _same(eng.render_two_pass(pk, bias, pk, bias, fr, bg, pix_index=px, workspace=ws, want_z=True), two, (name, tier, "workspace"))
            assert two[2].data_ptr() != ws["z"].data_ptr()
            u8 = eng.render_two_pass(pk, bias, pk, bias, fr, bg, pix_index=px, u8=True)
            assert torch.equal(u8[0], eng.to8b(two[0])) and (fields == 1 or torch.equal(u8[1], eng.to8b(two[1])))
