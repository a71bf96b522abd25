"""CPU-only: the blend decoder of tests/blend_scene.py is not vacuous, and the rounding model of the 16-bit tiers checks itself.

1. Conditions (not measurements) the oracle must meet on the 93 rays of frame 2, two fields, at 32 and at 64 coarse samples - the
   reasons tests/test_gpu_blend.py exists.  At (x 0.03, - 18) the oracle gives 93 / 28 / 31 rays, 26 argmax bins at 32 samples and
   gradient shares 0.997 / 0.92.  The fixtures' decoder fails the first and the fourth condition: its composite is opaque.
2. The rounding model (test_pack_plan.emulate with its operand-rounding hook, on blend_scene.DenseReader): the dense reader equals
   the pack plan's, the 16-bit encodings are the oracle's up to the f32 rounding of its arguments, and the model with its
   activations rounded toward zero separates from the nearest-even one by more than the gate the GPU test derives from it."""
import numpy as np
import pytest
import torch

import blend_scene as B
import dfa_oracle as O
import test_pack_plan as tpp


@pytest.fixture(scope="module")
def orc(scene, states, latents, golden):
    return B.Oracle(scene, B.blend_state(states), latents, golden("g7_frame_coarse"))


@pytest.fixture(scope="module")
def orc_fixture(scene, states, latents, golden):
    return B.Oracle(scene, states["decoder"], latents, golden("g7_frame_coarse"))


def _mid(x):
    return int(((x >= 0.1) & (x <= 0.9)).sum())


def test_blend_state_changes_three_tensors_only(states):
    st = B.blend_state(states)
    changed = sorted(k for k, v in states["decoder"].items() if not np.array_equal(v, st[k]))
    assert changed == ["fc_in_torso.weight", "fc_p_skips_torso.0.weight", "sigma_out.bias"]
    assert list(st) == list(states["decoder"]) and all(st[k].dtype == np.float32 for k in st)
    assert st["sigma_out.bias"][0] == np.float32(states["decoder"]["sigma_out.bias"][0] + np.float32(B.SIGMA_SHIFT))
    pix = B.ray_indices({"H": 450, "W": 450})
    assert len(pix) == 93 and 93 % 4 != 0 and 93 % 8 != 0 and len(np.unique(pix)) == 93


@pytest.mark.parametrize("nc", [32, 64])
def test_the_two_fields_share_the_rays(orc, nc):
    f = B.scene_figures(orc, nc)
    print(f"blend decoder, {nc} coarse samples: composite opacity in [0.1, 0.9] on {_mid(f['acc_com'])} rays, head share in [0.1, 0.9] "
          f"on {_mid(f['head_share'])}, head opacity in [0.1, 0.9] on {_mid(f['acc_head'])}, {len(f['argmax_bins'])} argmax bins")
    assert f["acc_com"].shape == (B.N_RAYS,)
    assert _mid(f["acc_com"]) >= 60
    assert _mid(f["head_share"]) >= 20
    assert _mid(f["acc_head"]) >= 20
    assert len(f["argmax_bins"]) >= nc / 4, f["argmax_bins"]


def test_no_two_rays_get_the_same_fine_depths_at_32_plus_32(orc):
    z_f = orc.render(32, 32, 2)[2]["z_fine"].numpy()
    assert z_f.shape == (B.N_RAYS, 32) and len(np.unique(z_f, axis=0)) == B.N_RAYS


def test_the_composite_gradient_reaches_the_deep_samples(orc):
    g_h, g_t = B.deep_gradient_share(orc)
    print(f"share of |d rgb_com / d sigma| behind the first 4 of 64 samples: head {g_h:.3f}, torso {g_t:.3f}")
    assert g_h >= 0.5 and g_t >= 0.5


def test_the_fixtures_decoder_fails_the_first_and_the_fourth_condition(orc_fixture):
    """why this file exists: with the fixtures' decoder no composite ray is translucent and the sampler of the composite image sees
    (almost) one inverse CDF - and four fifths of the composite's gradient sit in the first 4 samples"""
    for nc in (32, 64):
        f = B.scene_figures(orc_fixture, nc)
        assert _mid(f["acc_com"]) < 60 and f["acc_com"].min() > 0.9, nc
        assert len(f["argmax_bins"]) < nc / 4, (nc, f["argmax_bins"])
    g_h, g_t = B.deep_gradient_share(orc_fixture)
    assert g_h < 0.5 and g_t < 0.5, (g_h, g_t)


def test_the_oracles_own_float32_error_in_a_weight_exceeds_the_projects_per_weight_gate(orc):
    """why tests/test_gpu_blend.py gates single weights at 4 x blend_scene.W_F64 and not at the project's 2e-6: the oracle in float64
    against itself in float32 at 32 coarse samples (where the difference is largest) differs by more than half that gate in both
    images - measured 5.04e-6 (head) and 1.77e-6 (composite); the recorded figures are these, up to what a GEMM's sum order moves"""
    z = orc.render(32, 0, 2)[2]["z_coarse"].numpy()
    r32, r64 = orc.at(z), B.oracle_f64(orc, z)
    for name, k in (("head", 1), ("com", 3)):
        d = float((r32[k].double() - r64[k]).abs().max())
        print(f"max |w_{name}(float64) - w_{name}(float32)| of the oracle at 32 + 0: {d:.3e} (recorded {B.W_F64[name]:.3e})")
        assert d > 0.5 * 2e-6 and 0.5 * B.W_F64[name] <= d <= 1.5 * B.W_F64[name], (name, d)
    assert float((r32[0].double() - r64[0]).abs().max()) < 0.5 * 5e-5 and float((r32[2].double() - r64[2]).abs().max()) < 0.5 * 5e-5


# ---- the rounding model -----------------------------------------------------------------------------------------------------------
def test_rounders():
    x = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -10 + 2.0 ** -12), 70000.0, 3e-8, 0.1])
    near, zero = B.rounder("f16")(x), B.rounder("f16", True)(x)
    assert near.tolist()[:4] == [1.0, 1.0, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -10)]            # ties to even
    assert np.isinf(near[4]) and near[6] == float(np.float16(0.1))
    assert zero.tolist()[:4] == [1.0, 1.0, 1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10)] and (np.abs(zero[5:]) <= np.abs(x[5:])).all()
    y = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -7 + 2.0 ** -9), 3.0e38, 0.1])
    near, zero = B.rounder("bf16")(y), B.rounder("bf16", True)(y)
    assert near.tolist()[:4] == [1.0, 1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7)]
    assert zero.tolist()[:4] == [1.0, 1.0, 1.0 + 2.0 ** -7, -(1.0 + 2.0 ** -7)]
    assert np.isfinite(near[4]) and abs(near[5] - 0.1) <= 0.1 * 2.0 ** -8 and 0 < zero[5] <= 0.1


def test_posenc16_is_the_oracles_encoding_up_to_its_argument_rounding(golden):
    """the oracle rounds fl32(2^i pi) * fl32(p / 2) before the sine (up to 2^-24 x 512 pi at the top octave); the 16-bit tiers' form
    scales by powers of two and takes the fraction: exact arguments"""
    g = golden("g3_decoder")
    p = g["p_64"][0, :48]
    ref = O.posenc(torch.from_numpy(p)[None], 10)[0].double().numpy()
    got = B.posenc16(p, 10)
    assert got.shape == ref.shape == (48, 60)
    assert np.abs(got - ref).max() <= 512 * np.pi * np.abs(p).max() * 2.0 ** -24 + 1e-6
    assert np.abs(got[:, :6] - ref[:, :6]).max() <= 1e-6


@pytest.mark.parametrize("field", [0, 1])
def test_dense_reader_feeds_emulate_what_the_pack_plan_does(field, golden, states, latents):
    """emulate with the rounding hook, driven by the packed stream's plan (16-bit tiers: one plan) and by the dense weights: the same
    numbers - and without the hook the dense reader reproduces golden G3 at test_plan_reproduces_reference_decoder's gates"""
    g = golden("g3_decoder")
    st = B.blend_state(states)
    zs, za = latents
    p = g["p_64"][0, :48]
    r = g["r_64"][0, :48]
    rnd = B.rounder("f16")
    pe, pev = rnd(B.posenc16(p, 10)), rnd(B.posenc16(r / np.linalg.norm(r, axis=-1, keepdims=True), 4))
    sig = (g["sig_torso"][0] if field else g["sig_aud"][0]).astype(np.float64)
    args = (st, pe, pev, sig, zs[0, field].astype(np.float64), za[0, field].astype(np.float64))
    dense = lambda flat: B.DenseReader(field, st, flat)
    f_a, s_a = tpp.emulate(1, field, *args, rnd=rnd)           # (tier 1's plan is the f16 tier's too: test_f16_tier_shares_the_bf16_plan)
    f_b, s_b = tpp.emulate(1, field, *args, rnd=rnd, reader=dense)
    np.testing.assert_allclose(f_b, f_a, atol=1e-12, rtol=0)
    np.testing.assert_allclose(s_b, s_a, atol=1e-10, rtol=0)
    # unrounded, on the fixtures' decoder, against golden G3
    pe = O.posenc(torch.from_numpy(p)[None], 10)[0].double().numpy()
    rt = torch.from_numpy(r)
    pev = O.posenc((rt / torch.norm(rt, dim=-1, keepdim=True))[None], 4)[0].double().numpy()
    sd = states["decoder"]
    feat, sigma = tpp.emulate(1, field, sd, pe, pev, *args[3:], reader=lambda flat: B.DenseReader(field, sd, flat))
    name = "torso" if field else "head"
    np.testing.assert_allclose(feat, g[f"feat_{name}_64"][0, :48], atol=2e-5, rtol=0)
    np.testing.assert_allclose(sigma, g[f"sigma_{name}_64"][0, :48], atol=2e-4, rtol=1e-5)


@pytest.mark.parametrize("tier", ["f16", "bf16"])
def test_the_model_separates_from_a_wrong_rounding(orc, tier):
    """the gate tests/test_gpu_blend.py sets for a 16-bit tier is 2 x the rms error of this model's render against the exact oracle.
    A tier whose activations were rounded toward zero instead of to nearest must not fit under it: that model's render differs from
    the nearest-even model's by more than the gate, in both images (32 coarse samples, the oracle's own depths)."""
    z = orc.render(32, 0, 2)[2]["z_coarse"].numpy()
    exact = orc.at(z)
    near = orc.integrate(z, *B.model_fields(orc, z, tier))
    zero = orc.integrate(z, *B.model_fields(orc, z, tier, toward_zero=True))
    for name, k in (("head", 0), ("com", 2)):
        rms, worst, psnr = B.image_errors(near[k].numpy(), exact[k].numpy())
        sep = B.image_errors(zero[k].numpy(), near[k].numpy())[0]
        print(f"{tier} model, rgb_{name}: rms {rms:.3e} (largest per-ray {worst:.3e}, {psnr:.1f} dB) against the exact oracle; the "
              f"toward-zero model differs from it by {sep:.3e} rms = {sep / rms:.1f} x")
        assert rms > 0 and sep > 2.0 * rms, (tier, name, sep, rms)
