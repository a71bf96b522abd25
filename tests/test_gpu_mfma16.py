"""The f16 tier on v_mfma_f32_16x16x32_f16 (csrc/dfn_layout.h "16x16x32"), on the GPU: the instruction's fragment maps, the decoder
on explicit points (two points per lane: P0 / P1 mix-ups, ragged tiles) and the fused renderer on a handful of rays against the exact
tier.  Gates: the f16 tier's existing ones - decoder max |d feat| < 2.5e-3 and rms d sigma < 0.06 against the reference golden
(test_gpu_parity), images >= 49.4 dB with max |d| < 2e-2 (test_gpu_parity, test_gpu_bench).

Per-sample weights: the fine depths of a ray follow the coarse weights continuously, so sample i of the f16 launch is not the point
sample i of the f32 launch is, and a weight divided by a moved sample spacing is no comparable number.  What both launches share bit
for bit are the coarse depths; the weight accumulated in front of each of them, A(c) = 1 - transmittance at c, is compared.  Its gate
is the f16 tier's existing per-sample gate carried through the integral: A = 1 - exp(-sum sigma_i dist_i), so |dA| <= (1 - A) sum
dist_i |d sigma_i| <= L * |d sigma| with L = (far - near) * |ray| the length of the ray inside the volume; with the decoder gate
(rms d sigma < 0.06) on every sample that is W_GATE = 0.06 * L, about 4e-2 - no image clause applies, a colour sum averages what
this integral adds up.  Measured on MI355X: 47.5 dB / max 2.04e-2 (64+128, head) to 77.1 dB, and the parent commit's 32x32x16
kernels give the same figures to every printed digit (profiles/mfma16_accuracy.txt): the statistic is the f16 tier's, not the MFMA
shape's.  A point pair swapped inside a tile puts a surface's density 16 samples away: A moves by the surface's opacity (0.3 to 1 on
these rays), an order above the gate.  The images keep the image gates.

Coarse-only launches (64+0, 32+0) evaluate the same points in both tiers - the depths are equal bit for bit - so there the weights
ARE compared sample by sample, at the f16 tier's image gates (>= 49.4 dB, max |d| < 2e-2); measured 71.7-82.1 dB, max 2.7e-3, again
the same with the parent's library."""
import numpy as np
import pytest
import torch

import dfa_oracle as O
from dfanerf import synth

pytestmark = pytest.mark.gpu
t = torch.from_numpy
PSNR_DB, MAX_ABS = 49.4, 2e-2


@pytest.fixture(scope="module")
def eng():
    from dfanerf import engine
    engine.require_gpu()
    return engine


def psnr(a, b):
    mse = float(((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean())
    return 99.0 if mse == 0 else -10.0 * np.log10(mse)


def test_mfma16_fragment_maps(eng):
    """A row / B column = lane & 15, k = 8 (lane >> 4) + e, D row 4 (lane >> 4) + j: full asymmetric integer operands"""
    d = eng.mfma16_layout_probe().cpu().numpy()
    i, k = np.arange(16), np.arange(32)
    A = ((7 * i[:, None] + 3 * k[None, :]) % 13 + 1).astype(np.float64)
    B = ((5 * k[:, None] + 11 * i[None, :]) % 17 + 1).astype(np.float64)
    want = A @ B
    assert not np.array_equal(want, want.T) and not np.array_equal(want, B.T @ A.T)
    assert np.array_equal(d.astype(np.float64), want)


@pytest.mark.parametrize("field", [0, 1])
def test_decoder_forward_distinct_directions_and_prefixes(eng, states, latents, golden, field):
    g = golden("g3_decoder")
    zs, za = latents
    P = O.params_to_torch(states["decoder"])
    flat = eng.flatten_state(states["decoder"], "cuda")
    pk = eng.PackedDecoder(flat, "f16", fields=(0, 1))
    p = t(g["p_64"])                                                         # [1, 256, 3]: four rays of 64 points
    n_pts = p.shape[1]
    gen = torch.Generator().manual_seed(29 + field)
    r = torch.randn(1, n_pts, 3, generator=gen) * torch.rand(1, n_pts, 1, generator=gen).add(0.2)      # a direction (and length) per point
    sig = t(g["sig_aud"]) if field == 0 else t(g["sig_torso"])
    with torch.no_grad():
        rf, rs = O.decoder_forward(P, p, r, t(zs)[:, field], t(za)[:, field], [sig, None] if field == 0 else sig,
                                   "head" if field == 0 else "torso")
    bias = pk.fold_single(field, sig[0].numpy(), zs[0, field], za[0, field])
    pc, rc = p[0].cuda(), r[0].cuda()
    feat, sigma = eng.decoder_forward(pk, field, bias, pc, rc)
    df = float((feat.cpu() - rf[0]).abs().max())
    ds = float(((sigma.cpu() - rs[0]) ** 2).mean().sqrt())
    print(f"f16 16x16x32 decoder, field {field}: max |d feat| {df:.2e}, rms d sigma {ds:.2e}")
    assert df < 2.5e-3 and ds < 0.06
    for n in (1, 15, 16, 17, 31, 33, 129):
        f, s = eng.decoder_forward(pk, field, bias, pc[:n], rc[:n])
        assert torch.equal(f, feat[:n]) and torch.equal(s, sigma[:n]), n


RAYS = 9          # f16: two workgroups of eight waves, seven of them idle


def _frame_inputs(eng, scene, n_coarse, n_fine, fields):
    H, W = scene["H"], scene["W"]
    idx = ((H // 2 + np.arange(RAYS) * 7 - 28) * W + W // 2 + np.arange(RAYS) * 5 - 20).astype(np.int32)      # across the head
    fr = eng.make_frame(H, W, scene["focal"], scene["cx"], scene["cy"], scene["poses"][2], scene["pose_body"], scene["near"],
                        scene["far"], ray_count=RAYS, n_coarse=n_coarse, n_fine=n_fine, fields=fields)
    bg = (t(scene["bg"]).float() / 255.0).reshape(-1, 3).cuda()
    return fr, bg, t(idx).cuda()


def _check_against_f32(eng, packs, scene, bias_of, n_coarse, n_fine, fields, what):
    fr, bg, idx = _frame_inputs(eng, scene, n_coarse, n_fine, fields)
    out = {}
    for tier, pk in packs.items():
        o = eng.render(pk, bias_of(pk), fr, bg, pix_index=idx, want_weights=True, want_z=True)
        out[tier] = [None if x is None else x.cpu().numpy().astype(np.float64) for x in o]
    zc = O.coarse_z(scene["near"], scene["far"], n_coarse).numpy()
    _, d_h = O.get_rays(scene["H"], scene["W"], scene["focal"], scene["poses"][2][:3, :4], scene["cx"], scene["cy"])
    _, d_t = O.get_rays(scene["H"], scene["W"], scene["focal"], scene["pose_body"][:3, :4], scene["cx"], scene["cy"])
    norms = torch.cat([d_h.reshape(-1, 3)[idx.cpu().long()].norm(dim=-1), d_t.reshape(-1, 3)[idx.cpu().long()].norm(dim=-1)])
    ray_len = (scene["far"] - scene["near"]) * float(norms.max())               # L of the module docstring
    S = n_coarse + n_fine
    for tier in out:
        z = out[tier][4]
        assert z.shape == (RAYS, S) and (np.diff(z, axis=1) >= 0).all()
        for ray in range(RAYS):                                                  # the coarse depths, bit for bit, in both tiers
            assert np.isin(zc.astype(np.float32), z[ray].astype(np.float32)).all(), (tier, ray)
    for k, name in ((0, "rgb_head"), (1, "rgb_com")):
        a, b = out["f16"][k], out["f32"][k]
        if b is None:
            assert a is None and fields == 1
            continue
        print(f"{what} {name}: PSNR {psnr(a, b):.1f} dB, max |d| {np.abs(a - b).max():.2e}")
        assert psnr(a, b) >= PSNR_DB and np.abs(a - b).max() < MAX_ABS, (what, name)
    if n_fine == 0:
        # coarse only: both tiers evaluate the SAME points (the depths are equal bit for bit), so the weights compare sample by
        # sample - at the f16 tier's image gates: a weight is a colour sum's term with colour 1
        assert np.array_equal(out["f16"][4], out["f32"][4])
        for k, name in ((2, "w_head"), (3, "w_com")):
            a, b = out["f16"][k], out["f32"][k]
            if b is None:
                continue
            print(f"{what} {name}: per-sample weights: PSNR {psnr(a, b):.1f} dB, max |d| {np.abs(a - b).max():.2e}; "
                  f"largest single weight {b.max():.2f}")
            assert b[:, :-1].max() > 0.05                                        # the rays do hit something in front of the background
            assert psnr(a, b) >= PSNR_DB and np.abs(a - b).max() < MAX_ABS, (what, name)
        return
    for k, name in ((2, "w_head"), (3, "w_com")):
        if out["f32"][k] is None:
            continue
        cum = {}
        for tier in out:
            w, z = out[tier][k], out[tier][4]
            assert np.isfinite(w).all() and abs(w.sum(1) - 1.0).max() < 1e-3, (tier, name)
            # sample i's weight belongs to [z_i, z_i+1): strictly before a coarse depth c (itself a sample of both launches) lie
            # exactly the intervals that end at or before c
            cum[tier] = np.stack([(w * (z < c)).sum(1) for c in zc.astype(np.float64)], 1)           # [ray][coarse depth]
        a, b = cum["f16"], cum["f32"]
        print(f"{what} {name}: accumulated weight at the coarse depths: PSNR {psnr(a, b):.1f} dB, max |d| {np.abs(a - b).max():.2e}; "
              f"largest single weight {out['f32'][k].max():.2f}")
        assert out["f32"][k].max() > 0.05                                         # the rays do hit something
        assert np.abs(a - b).max() < 0.06 * ray_len, (what, name)


@pytest.fixture(scope="module")
def packs256(eng, states):
    flat = eng.flatten_state(states["decoder"], "cuda")
    return {tier: eng.PackedDecoder(flat, tier, fields=(0, 1)) for tier in ("f32", "f16")}


@pytest.mark.parametrize("fields", [1, 2])
@pytest.mark.parametrize("n_coarse,n_fine", [(64, 128), (32, 32), (64, 0), (32, 0)])
def test_render_nine_rays_against_the_f32_tier(eng, packs256, scene, latents, golden, n_coarse, n_fine, fields):
    gc = golden("g7_frame_coarse")
    zs, za = latents
    bias_of = lambda pk: pk.fold(gc["signal"][0], gc["signal_torso"].reshape(-1) if fields == 2 else None, zs[0], za[0])
    _check_against_f32(eng, packs256, scene, bias_of, n_coarse, n_fine, fields, f"{n_coarse}+{n_fine}, {fields} field(s)")


def test_render_nine_rays_128_wide_decoder(eng, scene, golden):
    """the native 128-wide program (half-length K over the hidden vector; the head's skip leaves the layers behind it at slab phase 16)"""
    g3 = golden("g3_decoder")
    flat = eng.flatten_state(synth.synth_decoder_state(0, z_dim=64, hidden=128), "cuda")
    packs = {tier: eng.PackedDecoder(flat, tier, fields=(0, 1), z_dim=64, width=128) for tier in ("f32", "f16")}
    zs, za = synth.synth_latents(0, z_dim=64)
    bias_of = lambda pk: pk.fold(g3["sig_aud"][0], g3["sig_torso"][0], zs[0], za[0])
    _check_against_f32(eng, packs, scene, bias_of, 64, 128, 2, "128 wide, 64+128, 2 fields")
