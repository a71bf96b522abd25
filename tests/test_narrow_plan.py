"""The 128-wide inference program (DFN_WIDTH_128 in the tier argument, include/dfanerf.h) - everything that needs no GPU: the
sizes of its pack plan, a numpy emulation of the narrow head / torso / listener programs driven by the plan alone against the
reference's own Decoder(hidden_size=128, z_dim=64) (golden G18), the refusals of every training entry point, and the host code
that selects the program (engine.select_width, PackedDecoder, Decoder.packed)."""
import numpy as np
import pytest
import torch

import dfa_oracle as O
from dfanerf import _lib, engine, synth
from test_pack_plan import flat_params, tile_feat

W128 = 0x200
# fragments of one pass (csrc/dfn_mlp.h Prog<TIER, 4>), 16-bit tiers (UPT = 2):
#   head  = IN 4 x 4 + 7 layers x 32 + skip 4 x 4 + view 5 tiles x (8 + 2) + out 8
#   torso = deformation field 104 + IN 4 x 8 + 7 x 32 + skip 4 x 8 + 50 + 8
FRAGS16 = {0: 16 + 7 * 32 + 16 + 5 * 10 + 8, 1: 104 + 32 + 224 + 32 + 50 + 8, 2: 16 + 7 * 32 + 16 + 5 * 10 + 8}
# f32 (UPT = 4): every k-length doubles
FRAGS32 = {0: 32 + 7 * 64 + 32 + 5 * 20 + 16, 1: 208 + 64 + 448 + 64 + 100 + 16, 2: 32 + 7 * 64 + 32 + 5 * 20 + 16}
E = {0: 4, 2: 8, 3: 8}
UPT = {0: 4, 2: 2, 3: 2}
SPLIT = {0: 1, 2: 1, 3: 2}


def slabs(frags):
    return (frags + 31) // 32


def test_fragment_counts_of_the_issue():
    assert FRAGS16[0] == 314 and slabs(314) == 10 and FRAGS16[1] == 450 and slabs(450) == 15


@pytest.mark.parametrize("field", [0, 1, 2])
def test_plan_sizes(field):
    L = _lib.lib
    for tier, frags in ((2, FRAGS16[field]), (3, 2 * FRAGS16[field]), (0, FRAGS32[field])):
        n = L.dfn_pack_plan(tier | W128, field, None, 0)
        assert n == slabs(frags) * 32 * 64 * E[tier], (tier, field, n, L.dfn_last_error())
        nbytes = L.dfn_packed_bytes(tier | W128, field)
        assert nbytes == slabs(frags) * 32 * 1024 and nbytes < L.dfn_packed_bytes(tier, field)
        plan = _lib.pack_plan(tier | W128, field)
        # ... and the plan's payload is exactly `frags` fragments: only slab padding behind them
        assert (plan[frags * 64 * E[tier]:] == -1).all() and (plan[(frags - 1) * 64 * E[tier]:frags * 64 * E[tier]] >= 0).any()
        # the bias blob does not change with the width (256-float strides; the fold kernel is the same)
        assert L.dfn_bias_floats(tier | W128, field) == L.dfn_bias_floats(tier, field) > 0
    # the f16 plan has the 16-bit (bf16-shaped) fragment map: 8 elements per lane, 2 k-units per tile - the first fragment of the
    # narrow plan IS the first fragment of the bf16 / f16 256-wide plan (rows 0..31 of the first layer over the first k-unit)
    p16, p16w = _lib.pack_plan(2 | W128, field), _lib.pack_plan(1, field)
    assert np.array_equal(p16[:512], p16w[:512])
    # f16x3: the same plan with every fragment twice in a row (hi, then lo')
    p3 = _lib.pack_plan(3 | W128, field)
    f16 = p16[:FRAGS16[field] * 512].reshape(-1, 512)
    assert np.array_equal(p3[:2 * FRAGS16[field] * 512].reshape(-1, 2, 512), np.repeat(f16[:, None, :], 2, axis=1))


def kslot_to_slot(tier, u, h, e):
    t, r = u // UPT[tier], (u % UPT[tier]) * E[tier] + e
    return 32 * t + tile_feat(h, r)


class Reader:
    """tests/test_pack_plan.py's Reader for the narrow plans (tiers 0 / 2 / 3): walks the packed stream in consumption order and
    rebuilds the dense weights of each tile group; remembers every flat index it was handed."""

    def __init__(self, tier, field, flat):
        self.tier, self.plan, self.flat, self.pos = tier, _lib.pack_plan(tier | W128, field), flat, 0

    def group(self, G, KU, nslots):
        W = np.zeros((32 * G, nslots))
        e_n = E[self.tier]
        for ku in range(KU):
            for g in range(G):
                for part in range(SPLIT[self.tier]):
                    frag = self.plan[self.pos:self.pos + 64 * e_n].reshape(64, e_n)
                    self.pos += 64 * e_n
                    if part:
                        assert np.array_equal(frag, prev)       # (hi, lo'): the same entries
                        continue
                    prev = frag
                    for lane in range(64):
                        i, h = lane & 31, lane >> 5
                        for e in range(e_n):
                            idx = frag[lane, e]
                            if idx >= 0:
                                W[32 * g + i, kslot_to_slot(self.tier, ku, h, e)] = self.flat[idx]
        return W

    def layer(self, OT, KU, nslots):
        return np.concatenate([self.group(2, KU, nslots) for _ in range(OT // 2)], 0)

    def layer_skip(self, OT, KU, nslots, KU2, nslots2):
        a, b = [], []
        for _ in range(OT // 2):
            a.append(self.group(2, KU, nslots))
            b.append(self.group(2, KU2, nslots2))
        return np.concatenate(a, 0), np.concatenate(b, 0)


def emulate(tier, field, st, pe, pev, sig, zs, za):
    """numpy restatement of mlp_head<TIER, 4> / mlp_torso<TIER, 4> (csrc/dfn_mlp.h) driven by the narrow plan: 4 output tiles per
    trunk layer, 4 x UPT k-units over the hidden vector, two feat_view pairs.  `st`: the decoder's tensors in the library's padded
    shapes (engine.padded_shape): the biases are read at [:128] - the first 128 entries of the 256-float vectors of the blob."""
    P = {k: np.asarray(v, np.float64) for k, v in st.items()}
    rd = Reader(tier, field, flat_params(st).astype(np.float64))
    u, H = UPT[tier], 128
    relu = lambda x: np.maximum(x, 0)
    N = pe.shape[0]
    pe64 = np.zeros((N, 64)); pe64[:, :60] = pe
    v32 = np.zeros((N, 32)); v32[:, :24] = pev
    fcz = (P["fc_z.weight"] @ zs + P["fc_z.bias"])[:H]
    fczs = (P["fc_z_skips.0.weight"] @ zs + P["fc_z_skips.0.bias"])[:H]
    fczv = (P["fc_z_view.weight"] @ za + P["fc_z_view.bias"])[:H]
    if field in (0, 2):
        nm = ("fc_in", "fc_p_skips.0") if field == 0 else ("fc_in_listener", "fc_p_skips_listener.0")
        b_in = P[nm[0] + ".bias"][:H] + fcz
        b_sk = P[nm[1] + ".bias"][:H] + fczs
        if field == 0:
            b_in = b_in + (P[nm[0] + ".weight"][:, 60:] @ sig)[:H]
            b_sk = b_sk + (P[nm[1] + ".weight"][:, 60:] @ sig)[:H]
        act = relu(pe64 @ rd.layer(4, 2 * u, 64).T + b_in)
        pvec, kup, nps = pe64, 2 * u, 64
    else:
        w = lambda n: P[f"deform_net.{n}.weight"]
        b = lambda n: P[f"deform_net.{n}.bias"]
        ve = relu(pe64 @ rd.layer(2, 2 * u, 64).T + b("blocks_embed.0") + w("blocks_embed.0")[:, 60:] @ sig)
        vs = relu(pe64 @ rd.layer(2, 2 * u, 64).T + b("blocks_signal.0") + w("blocks_signal.0")[:, 60:] @ sig)
        ve = relu(ve @ rd.layer(2, 2 * u, 64).T + b("blocks_embed.1"))
        vs = relu(vs @ rd.layer(2, 2 * u, 64).T + b("blocks_signal.1"))
        ve = relu(ve @ rd.layer(2, 2 * u, 64).T + b("blocks_embed.2"))
        vs = relu(vs @ rd.layer(2, 2 * u, 64).T + b("blocks_signal.2"))
        w3, wsk = rd.layer_skip(2, 2 * u, 64, 2 * u, 64)
        ve = relu(ve @ w3.T + b("blocks_embed.3")) + b("fc_embed_skips.0") + pe64 @ wsk.T
        vs = relu(vs @ rd.layer(2, 2 * u, 64).T + b("blocks_signal.3")) + b("fc_signal_skips.0") + \
            w("fc_signal_skips.0") @ sig
        ve = relu(ve @ rd.layer(2, 2 * u, 64).T + b("blocks_embed.4"))
        vs = relu(vs @ rd.layer(2, 2 * u, 64).T + b("blocks_signal.4"))
        eo = ve @ rd.layer(2, 2 * u, 64).T + np.pad(b("out_embed"), (0, 4))
        so = vs @ rd.layer(2, 2 * u, 64).T + np.pad(b("out_signal") + sig, (0, 22))
        pd = np.concatenate([eo + pe64, so], 1)
        act = relu(pd @ rd.layer(4, 4 * u, 128).T + P["fc_in_torso.bias"][:H] + fcz)
        b_sk = P["fc_p_skips_torso.0.bias"][:H] + fczs
        pvec, kup, nps = pd, 4 * u, 128
    for l in range(3):
        act = relu(act @ rd.layer(4, 4 * u, H).T + P[f"blocks.{l}.bias"][:H])
    w4, wsk = rd.layer_skip(4, 4 * u, H, kup, nps)
    act = relu(act @ w4.T + P["blocks.3.bias"][:H]) + b_sk + pvec @ wsk.T
    for l in range(4, 7):
        act = relu(act @ rd.layer(4, 4 * u, H).T + P[f"blocks.{l}.bias"][:H])
    rows = []
    for tg in range(2):
        rows.append(act @ rd.group(2, 4 * u, H).T + v32 @ rd.group(2, u, 32).T)
    hid = relu(np.concatenate(rows, 1) + P["feat_view.bias"][:H] + fczv + P["fc_view.bias"][:H])
    sg = act @ rd.group(1, 4 * u, H).T + v32 @ rd.group(1, u, 32).T
    sigma = sg[:, 0] + P["sigma_out.bias"][0]
    assert np.abs(sg[:, 1:]).max() == 0          # rows 1..31 of the sigma tile are structural zeros
    out = hid @ rd.group(1, 4 * u, H).T
    assert np.abs(out[:, 3:]).max() == 0
    feat = 1 / (1 + np.exp(-(out[:, :3] + P["feat_out.bias"])))
    frag_elems = 64 * E[tier]
    assert rd.pos % frag_elems == 0 and (rd.plan[rd.pos:] == -1).all()     # only slab padding remains unread
    assert rd.pos == SPLIT[tier] * (FRAGS32 if tier == 0 else FRAGS16)[field] * frag_elems
    return feat, sigma


@pytest.fixture(scope="module")
def narrow_state():
    """G18's network - the reference's Decoder(hidden_size=128, z_dim=64) - in the library's padded shapes, plus the
    (offset, shape) of every tensor in the flat vector"""
    st = synth.synth_decoder_state(0, z_dim=64, hidden=128)
    pad, layout, off = {}, {}, 0
    for k, v in st.items():
        want = engine.padded_shape(k, v.shape)
        full = np.zeros(want, np.float32)
        full[tuple(slice(0, n) for n in v.shape)] = v
        pad[k] = full
        layout[k] = (off, want, v.shape)
        off += full.size
    assert off == _lib.N_DECODER_PARAMS
    return pad, layout


@pytest.mark.parametrize("tier", [0, 2])
@pytest.mark.parametrize("field", [0, 1, 2])
def test_narrow_plan_reproduces_reference_decoder(tier, field, golden, narrow_state):
    g, g3 = golden("g18_n_feat_128"), golden("g3_decoder")
    st, _ = narrow_state
    zs, za = [np.pad(z, ((0, 0), (0, 0), (0, 192))) for z in synth.synth_latents(0, z_dim=64)]
    p, r = torch.from_numpy(g3["p_64"][:, :48]), torch.from_numpy(g3["r_64"][:, :48])
    pe = O.posenc(p, 10)[0].double().numpy()
    pev = O.posenc(r / torch.norm(r, dim=-1, keepdim=True), 4)[0].double().numpy()
    fi = 1 if field == 1 else 0
    sig = {0: g3["sig_aud"][0], 1: g3["sig_torso"][0], 2: None}[field]
    feat, sigma = emulate(tier, field, st, pe, pev, None if sig is None else sig.astype(np.float64),
                          zs[0, fi].astype(np.float64), za[0, fi].astype(np.float64))
    name = {0: "head", 1: "torso", 2: "listener"}[field]
    # (the gates of test_pack_plan.test_plan_reproduces_reference_decoder)
    np.testing.assert_allclose(feat, g[f"feat_{name}"][0, :48], atol=2e-5, rtol=0)
    np.testing.assert_allclose(sigma, g[f"sigma_{name}"][0, :48], atol=2e-4, rtol=1e-5)


@pytest.mark.parametrize("tier", [0, 2, 3])
@pytest.mark.parametrize("field", [0, 1, 2])
def test_narrow_plan_stays_below_128(tier, field, narrow_state):
    """no plan entry references a row or column >= 128 of a hidden-sized tensor, and every entry of G18's network that the
    256-wide plan references and that is non-zero is in the narrow plan too (nothing of a 128-wide network is dropped)"""
    st, layout = narrow_state
    plan = _lib.pack_plan(tier | W128, field)
    used = np.unique(plan[plan >= 0])
    seen = 0
    for k, (off, want, orig) in layout.items():
        idx = used[(used >= off) & (used < off + int(np.prod(want)))] - off
        if idx.size == 0:
            continue
        seen += idx.size
        if len(want) == 2:
            rows, cols = idx // want[1], idx % want[1]
            if k.startswith(engine._HID_ROWS):
                assert rows.max() < 128, (k, rows.max())
            if k.startswith(engine._HID_COLS):
                assert cols.max() < 128, (k, cols.max())
    assert seen == used.size
    flat = flat_params(st)
    wide = _lib.pack_plan(tier, field)
    wide = np.unique(wide[wide >= 0])
    dropped = np.setdiff1d(wide, used)
    assert dropped.size > 0 and not flat[dropped].any()
    assert np.setdiff1d(used, wide).size == 0


def test_training_entry_points_refuse_the_flag():
    L, N, one = _lib.lib, None, 4096
    err = lambda: L.dfn_last_error()
    fr = _lib.DfnFrame()
    fr.n_coarse, fr.n_fine, fr.fields, fr.ray_count, fr.H, fr.W = 64, 0, 2, 8, 4, 4
    for tier in (0 | W128, 1 | W128, 2 | W128):
        a16 = (tier, _lib.C.byref(fr), one, one, one, one, one, N, one, one, one, one, one, one, one, one)
        loss = _lib.DfnTrainLoss(one, one, one, one, one, one)
        calls = {
            "dfn_packed_bwd_bytes": lambda: L.dfn_packed_bwd_bytes(tier, 0),
            "dfn_pack_weights_bwd": lambda: L.dfn_pack_weights_bwd(tier, 0, one, one, N),
            "dfn_train_prepare": lambda: L.dfn_train_prepare(tier, one, one, one, one, one, one, one, one, one, one, one, N),
            "dfn_train_fwd": lambda: L.dfn_train_fwd(*a16, N),
            "dfn_train_fwd_hier": lambda: L.dfn_train_fwd_hier(*a16, one, one, N),
            "dfn_train_fwd_loss": lambda: L.dfn_train_fwd_loss(*a16, _lib.C.byref(loss), N),
            "dfn_train_fwd_hier_loss": lambda: L.dfn_train_fwd_hier_loss(*a16, one, one, _lib.C.byref(loss), N),
            "dfn_mlp_bwd": lambda: L.dfn_mlp_bwd(tier, 0, one, one, one, one, 64, one, N),
            "dfn_weight_grad": lambda: L.dfn_weight_grad(tier, 0, one, one, 64, one, one, N),
            "dfn_bias_grad": lambda: L.dfn_bias_grad(tier, 0, one, 64, one, one, N),
            "dfn_weight_bias_grad": lambda: L.dfn_weight_bias_grad(tier, 0, one, one, 64, one, one, one, N),
            "dfn_weight_bias_grad_fmt": lambda: L.dfn_weight_bias_grad_fmt(tier, 0, 1, one, one, 64, one, one, one, N),
            "dfn_weight_bias_grad_partials": lambda: L.dfn_weight_bias_grad_partials(tier, 0, 1, one, one, 64, one, one, N),
            "dfn_weight_bias_grad_partials_part": lambda: L.dfn_weight_bias_grad_partials_part(tier, 0, 1, one, one, 64, one, one, 3, N),
            "dfn_weight_bias_grad_reduce": lambda: L.dfn_weight_bias_grad_reduce(tier, 0, 64, one, one, one, N),
            "dfn_fold_bias_bwd": lambda: L.dfn_fold_bias_bwd(tier, 0, one, one, one, one, one, one, N, N),
            "dfn_signal_grad": lambda: L.dfn_signal_grad(tier, 0, one, one, 64, one, one, N),
            "dfn_decoder_train_fwd": lambda: L.dfn_decoder_train_fwd(tier, 0, one, one, one, one, 32, one, one, one, one, one, N),
        }
        for name, call in calls.items():
            assert call() == -1 and b"DFN_WIDTH_128" in err(), (name, tier, err())
    # bf16 is the training tier and stays padded: the inference entry points refuse the flag with it
    assert L.dfn_packed_bytes(1 | W128, 0) < 0 and b"DFN_WIDTH_128" in err()
    assert L.dfn_pack_plan(1 | W128, 0, None, 0) < 0 and b"DFN_WIDTH_128" in err()
    assert L.dfn_pack_weights(1 | W128, 0, one, one, N) == -1 and b"DFN_WIDTH_128" in err()
    assert L.dfn_bias_floats(1 | W128, 0) < 0 and L.dfn_fold_bias(1 | W128, 0, one, one, one, one, one, N) == -1
    assert L.dfn_decoder_fwd(1 | W128, 0, one, one, one, one, 4, one, one, N) == -1 and b"DFN_WIDTH_128" in err()
    fr.n_fine = 128
    assert L.dfn_render_fwd(1 | W128, _lib.C.byref(fr), one, one, one, one, one, N, N, one, one, N, N, N, N) == -1 and b"DFN_WIDTH_128" in err()
    assert L.dfn_render_fwd_u8(1 | W128, _lib.C.byref(fr), one, one, one, one, one, N, N, one, one, N) == -1 and b"DFN_WIDTH_128" in err()
    # ... and accept it in the inference tiers: the ordinary argument checks answer (here: no weights), not the flag's
    assert L.dfn_render_fwd(2 | W128, _lib.C.byref(fr), N, N, one, N, one, N, N, one, N, N, N, N, N) == -1 and b"DFN_WIDTH_128" not in err()
    assert L.dfn_decoder_fwd(3 | W128, 0, one, one, N, one, 4, one, one, N) == -1 and b"DFN_WIDTH_128" not in err()
    assert _lib.WIDTH_128 == W128


# ---- host selection (no device: the library calls of PackedDecoder are recorded, not made) ---------------------------------
def test_select_width(monkeypatch):
    monkeypatch.delenv("DFN_WIDTH", raising=False)
    for tier in ("f32", "f16", "f16x3"):
        assert engine.select_width(128, tier) == 128 and engine.select_width(64, tier) == 128
        assert engine.select_width(129, tier) == 256 and engine.select_width(256, tier) == 256
    assert engine.select_width(128, "bf16") == 256
    monkeypatch.setenv("DFN_WIDTH", "256")
    assert engine.select_width(128, "f16") == 256
    monkeypatch.setenv("DFN_WIDTH", "128")
    assert engine.select_width(128, "f16") == 128
    with pytest.raises(ValueError, match="truncate"):
        engine.select_width(256, "f16")
    with pytest.raises(ValueError):
        engine.select_width(128, "bf16")
    monkeypatch.setenv("DFN_WIDTH", "192")
    with pytest.raises(ValueError):
        engine.select_width(128, "f16")
    monkeypatch.delenv("DFN_WIDTH")
    with pytest.raises(ValueError):
        engine.select_width(256, "f32", force="128")


class _FakeLib:
    """records the tier argument of every library call PackedDecoder / engine.render make"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(tier, *a):
            self.calls.append((name, tier))
            return 4096 if name in ("dfn_packed_bytes", "dfn_bias_floats") else 0
        return f


@pytest.fixture
def fake_engine(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(engine, "lib", fake)
    monkeypatch.setattr(engine, "require_gpu", lambda: None)
    monkeypatch.setattr(engine, "_stream", lambda: None)
    monkeypatch.delenv("DFN_WIDTH", raising=False)
    return fake


def test_packed_decoder_carries_the_flag(fake_engine):
    flat = torch.zeros(8)
    pk = engine.PackedDecoder(flat, "f32", fields=(0, 1), width=128)
    assert pk.width == 128 and pk.tier == 0 and pk.tier_arg == W128
    pk.fold(torch.zeros(96), torch.zeros(42), torch.zeros(2, 256), torch.zeros(2, 256))
    pk.fold_single(2, None, torch.zeros(256), torch.zeros(256))
    fr = engine.make_frame(4, 4, 1.0, 2.0, 2.0, np.eye(4), np.eye(4), 0.1, 1.0, ray_count=4, fields=2)
    bias = torch.zeros(8192)
    engine.render(pk, bias, fr, torch.zeros(16, 3))
    engine.render_u8(pk, bias, fr, torch.zeros(16, 3))
    engine.decoder_forward(pk, 0, bias, torch.zeros(4, 3), torch.ones(4, 3))
    names = {n for n, _ in fake_engine.calls}
    assert {"dfn_packed_bytes", "dfn_pack_weights", "dfn_bias_floats", "dfn_fold_bias", "dfn_render_fwd", "dfn_render_fwd_u8",
            "dfn_decoder_fwd"} <= names
    assert all(t == W128 for _, t in fake_engine.calls), fake_engine.calls
    fake_engine.calls.clear()
    pk = engine.PackedDecoder(flat, "f16x3", fields=(0,))            # the default stays the padded program
    assert pk.width == 256 and pk.tier_arg == 3 and all(t == 3 for _, t in fake_engine.calls)
    with pytest.raises(ValueError):
        engine.PackedDecoder(flat, "bf16", width=128)
    with pytest.raises(ValueError):
        engine.PackedDecoder(flat, "f32", width=192)


def _decoder(hidden, monkeypatch):
    from dfanerf.decoder import Decoder
    dec = Decoder(z_dim=64, hidden_size=hidden, dim_signal=96, use_deformation_field=True)
    monkeypatch.setattr(engine, "flatten_state", lambda state, device: torch.zeros(8))
    return dec


@pytest.mark.parametrize("hidden,tier,env,want", [(128, "f32", None, 128), (128, "f16", None, 128), (128, "f16x3", None, 128),
                                                  (64, "f16", None, 128), (129, "f32", None, 256), (256, "f16", None, 256),
                                                  (128, "f16", "256", 256), (128, "bf16", None, 256)])
def test_decoder_packed_selects_the_program(fake_engine, monkeypatch, hidden, tier, env, want):
    if env is not None:
        monkeypatch.setenv("DFN_WIDTH", env)
    pk = _decoder(hidden, monkeypatch).packed(tier)
    assert pk.width == want and pk.tier_arg == engine.TIERS[tier] | (W128 if want == 128 else 0)
    assert all(t == pk.tier_arg for _, t in fake_engine.calls)


def test_forcing_128_on_a_wider_decoder_raises(fake_engine, monkeypatch):
    monkeypatch.setenv("DFN_WIDTH", "128")
    with pytest.raises(ValueError):
        _decoder(256, monkeypatch).packed("f16")
    assert _decoder(128, monkeypatch).packed("f16").width == 128
