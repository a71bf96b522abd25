"""CPU-only checks of the f16x3 tier's host side (split f16 operands, include/dfanerf.h DFN_TIER_F16X3): the stream sizes, the
pack plan - every f16 fragment followed by its lo' twin - and the kernel's split dataflow emulated in numpy from that plan
(test_pack_plan.emulate, every GEMM operand split into hi = f16(x) and lo' = f16((x - hi) 2^11), hi.hi + 2^-11 (hi.lo' + lo'.hi)),
which must reproduce golden G3 at the f32 tier's gates.  No GPU."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import dfa_oracle as O
import test_pack_plan as tpp
from dfanerf import _lib
from dfanerf.run_nerf import check_supported

TIER_F16X3 = 3


def test_tier_constant():
    assert _lib.TIER_F16X3 == TIER_F16X3


@pytest.mark.parametrize("field", [0, 1, 2])
def test_packed_bytes_twice_the_f16_tier(field):
    assert _lib.lib.dfn_packed_bytes(TIER_F16X3, field) == 2 * _lib.lib.dfn_packed_bytes(2, field)
    assert _lib.lib.dfn_bias_floats(TIER_F16X3, field) == _lib.lib.dfn_bias_floats(2, field)


@pytest.mark.parametrize("field", [0, 1, 2])
def test_plan_interleaves_hi_and_lo_fragments_of_the_f16_plan(field):
    p16, p3 = _lib.pack_plan(2, field), _lib.pack_plan(TIER_F16X3, field)
    f16 = p16.reshape(-1, 512)
    used = int(np.nonzero((f16 >= 0).any(1))[0].max()) + 1           # fragments before the slab padding
    f3 = p3.reshape(-1, 2, 512)
    assert np.array_equal(f3[:used, 0], f16[:used]) and np.array_equal(f3[:used, 1], f16[:used])
    assert (p3[2 * used * 512:] == -1).all()


def join(x):
    """the value a split operand stands for, hi + 2^-11 lo' (what the kernel's Vec::get returns)"""
    hi, lo = split(x)
    return hi + lo / 2048.0


def split(x):
    """x (float32 values) -> (hi, lo') as float64 arrays of f16 values, the way the kernels and pack_kernel split"""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


class SplitW:
    """a dense weight block held as (hi, lo'): `x @ w.T` is the f16x3 product of split x and split w"""
    __array_ufunc__ = None           # numpy hands `ndarray @ SplitW` to __rmatmul__

    def __init__(self, hi, lo):
        self.hi, self.lo = hi, lo

    @property
    def T(self):
        return self

    def __rmatmul__(self, x):
        xh, xl = split(x)
        return xh @ self.hi.T + (xh @ self.lo.T + xl @ self.hi.T) / 2048.0


class SplitReader(tpp.Reader):
    """tpp.Reader for the f16x3 stream: each fragment pair (hi, lo') holds the same plan indices; the weights come back split"""

    def __init__(self, tier, field, flat):
        super().__init__(tier, field, flat)
        self.flat = np.asarray(flat, np.float32)

    def raw(self, G, KU, nslots):
        Wi = np.full((32 * G, nslots), -1, np.int64)
        for ku in range(KU):
            for g in range(G):
                hi = self.plan[self.pos:self.pos + 512].reshape(64, 8)
                lo = self.plan[self.pos + 512:self.pos + 1024].reshape(64, 8)
                assert np.array_equal(hi, lo)
                self.pos += 1024
                for lane in range(64):
                    i, h = lane & 31, lane >> 5
                    for e in range(8):
                        Wi[32 * g + i, tpp.kslot_to_slot(self.tier, ku, h, e)] = hi[lane, e]
        return Wi

    def wrap(self, Wi):
        W = np.where(Wi >= 0, self.flat[np.maximum(Wi, 0)], np.float32(0.0))
        return SplitW(*split(W))

    def group(self, G, KU, nslots):
        return self.wrap(self.raw(G, KU, nslots))

    def layer(self, OT, KU, nslots):
        return self.wrap(np.concatenate([self.raw(2, KU, nslots) for _ in range(OT // 2)], 0))

    def layer_skip(self, OT, KU, nslots, KU2, nslots2):
        a, b = [], []
        for _ in range(OT // 2):
            a.append(self.raw(2, KU, nslots))
            b.append(self.raw(2, KU2, nslots2))
        return self.wrap(np.concatenate(a, 0)), self.wrap(np.concatenate(b, 0))


@pytest.mark.parametrize("field", [0, 1, 2])
def test_split_dataflow_from_the_plan_reproduces_reference_decoder(field, golden, states, latents, monkeypatch):
    """The f16x3 scheme on weights and activations alike, driven by the tier's own pack plan, against golden G3 at the f32
    tier's gates (feat 1e-5, sigma 2e-4 + 1e-5 relative)."""
    monkeypatch.setattr(tpp, "Reader", SplitReader)
    monkeypatch.setitem(tpp.E, TIER_F16X3, 8)
    monkeypatch.setitem(tpp.UPT, TIER_F16X3, 2)
    g = golden("g3_decoder")
    zs, za = latents
    p, r = torch.from_numpy(g["p_64"][:, :48]), torch.from_numpy(g["r_64"][:, :48])
    # the encodings as the kernel holds them: split (the GEMMs split them again to the same hi / lo'), and the torso's residual
    # deform(p) + p adds this value, not the exact f32 encoding (dfn_mlp.h mlp_torso)
    pe = join(O.posenc(p, 10)[0].numpy())
    pev = join(O.posenc(r / torch.norm(r, dim=-1, keepdim=True), 4)[0].numpy())
    fi = 1 if field == 1 else 0
    sig = {0: g["sig_aud"][0], 1: g["sig_torso"][0], 2: None}[field]
    feat, sigma = tpp.emulate(TIER_F16X3, field, states["decoder"], pe, pev, None if sig is None else sig.astype(np.float64),
                              zs[0, fi].astype(np.float64), za[0, fi].astype(np.float64))
    name = {0: "head", 1: "torso", 2: "listener"}[field]
    rf, rs = g[f"feat_{name}_64"][0, :48], g[f"sigma_{name}_64"][0, :48]
    print(f"f16x3 emulation field {field}: max|dfeat| {np.abs(feat - rf).max():.2e}  max|dsigma| {np.abs(sigma - rs).max():.2e}")
    np.testing.assert_allclose(feat, rf, atol=1e-5, rtol=0)
    np.testing.assert_allclose(sigma, rs, atol=2e-4, rtol=1e-5)


def _args(tier):
    return argparse.Namespace(dim_signal=96, z_dim=256, n_feat=256, N_samples=64, hierarchical=False, N_importance=128,
                              n_object=1, hip_tier=tier, hip_train_act="fp4")


def test_cli_accepts_f16x3_and_still_refuses_unknown_tiers():
    check_supported(_args("f16x3"))
    for tier in ("f32", "f16", "bf16", "auto"):
        check_supported(_args(tier))
    with pytest.raises(SystemExit, match="f16x3"):
        check_supported(_args("f16x4"))


def test_training_entry_points_refuse_the_tier():
    """every argument valid but the tier (zero rays / points: the f32 tier returns DFN_OK before any device work), so the tier
    is what refuses; dfn_fold_bias_bwd accepts the inference tiers like dfn_fold_bias (the bias blob is shared by all tiers)"""
    L = _lib.lib
    assert L.dfn_packed_bwd_bytes(TIER_F16X3, 0) == -1
    assert L.dfn_packed_bwd_bytes(1, 0) > 0
    buf = np.zeros(1024, np.float32)
    p = buf.ctypes.data
    fr = _lib.DfnFrame()
    fr.H, fr.W, fr.ray_count, fr.n_coarse, fr.n_fine, fr.fields = 8, 8, 0, 64, 0, 2
    for tier, want in ((0, 0), (1, 0), (2, -1), (TIER_F16X3, -1)):
        assert L.dfn_train_fwd(tier, C.byref(fr), *([p] * 15)) == want, tier
        assert L.dfn_decoder_train_fwd(tier, 0, p, p, p, p, 0, p, p, p, p, p, None) == want, tier
    assert b"dfn_decoder_train_fwd: bad argument" in L.dfn_last_error()
    fr.n_fine = 128
    for tier, want in ((0, 0), (TIER_F16X3, -1)):
        assert L.dfn_train_fwd_hier(tier, C.byref(fr), *([p] * 17)) == want, tier
