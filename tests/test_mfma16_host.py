"""CPU-only checks of the f16 tier's 16x16x32 dataflow (csrc/dfn_layout.h "16x16x32"): the kernels' fragment reads restated in
numpy from the lane maps the library is compiled with (dfn_mfma16_map) and the unchanged pack plan of the 16-bit tiers.

Lane l = (i = l & 15, k-group g = l >> 4).  Per K = 32 step of a tile group the kernel takes the LDS image of 2 G stream fragments
(each written by one LDS-DMA piece, lane L fetching the 16-byte slot dma[L]), and every lane reads one 16-byte slot per (tile, T) as
the A operand of two MFMAs: MFMA row i of half T is tile row (i & 7) + 16 (i >> 3) + 8 T, and the slot's eight elements must be the
weights of that row against exactly the eight input features feat[l] the lane's k-group holds of every 32-feature tile."""
import numpy as np
import pytest
import torch

import dfa_oracle as O
import test_pack_plan as tpp
from dfanerf import _lib

FRAG_SLOTS = 64          # 16-byte slots per 1-KiB fragment


class _Map(dict):
    """the library's lane tables, fetched on first use (collection must not need them)"""

    def __missing__(self, key):
        self.update(_lib.mfma16_map())
        return dict.__getitem__(self, key)


M = _Map()


def m16_row(i, T):
    return (i & 7) + 16 * (i >> 3) + 8 * T


class M16Reader:
    """tests/test_pack_plan.Reader for the 16x16x32 dataflow: the dense weights of a tile group as the f16 kernels' MFMAs see them"""

    def __init__(self, field, flat):
        self.plan, self.flat, self.frag = _lib.pack_plan(2, field), flat, 0

    def image(self, n):
        """LDS image of the next n stream fragments, [n * 64 slots][8 plan entries]: LDS slot L of a fragment = stream slot dma[L] / 16"""
        frags = self.plan[self.frag * 512:(self.frag + n) * 512].reshape(n, FRAG_SLOTS, 8)
        self.frag += n
        return frags[:, M["dma"] // 16].reshape(n * FRAG_SLOTS, 8)

    def group(self, G, KU, nslots):
        assert KU % 2 == 0
        W = np.zeros((32 * G, nslots))
        rd = M["rd2"] if G == 2 else M["rd1"]
        lanes = np.arange(64)
        for v in range(KU // 2):
            img = self.image(2 * G)
            for j in range(2 * G):
                tile, T = (j >> 1, j & 1) if G == 2 else (0, j)
                assert (rd[j] % 16 == 0).all() and (rd[j] >= 0).all() and (rd[j] < 2 * G * 1024).all()
                idx = img[rd[j] // 16]                                           # [lane][e]
                rows = (32 * tile + m16_row(lanes & 15, T))[:, None].repeat(8, 1)
                cols = 32 * v + M["feat"]
                ok = idx >= 0
                assert (W[rows[ok], cols[ok]] == 0).all()                         # no (row, feature) is read twice
                W[rows[ok], cols[ok]] = self.flat[idx[ok]]
        return W

    def layer(self, OT, KU, nslots):
        return np.concatenate([self.group(2, KU, nslots) for _ in range(OT // 2)], 0)

    def layer_skip(self, OT, KU, nslots, KU2, nslots2):
        a, b = [], []
        for _ in range(OT // 2):
            a.append(self.group(2, KU, nslots))
            b.append(self.group(2, KU2, nslots2))
        return np.concatenate(a, 0), np.concatenate(b, 0)


class BothReaders:
    """Every tile group through the 32x32x16 walk (tests/test_pack_plan.Reader) and the 16x16x32 one, on parameter INDICES: the two
    dense index matrices must be the same matrix - every slot (i, g, T, v) of the new fragments carries the parameter of output row
    m16_row(i, T) against the feature feat[lane][e] of source tile v, and nothing of the stream is dropped.  Returns real weights."""

    def __init__(self, field, flat):
        ids = np.arange(1, _lib.N_DECODER_PARAMS + 1, dtype=np.float64)
        self.old, self.new, self.flat, self.groups = tpp.Reader(1, field, ids), M16Reader(field, ids), flat, 0

    def group(self, G, KU, nslots):
        a, b = self.old.group(G, KU, nslots), self.new.group(G, KU, nslots)
        assert np.array_equal(a, b), (self.groups, G, KU)
        assert self.old.pos == self.new.frag * 512
        self.groups += 1
        ids = a.astype(np.int64)
        return np.where(ids > 0, self.flat[np.maximum(ids - 1, 0)], 0.0)

    layer = M16Reader.layer
    layer_skip = M16Reader.layer_skip


@pytest.mark.parametrize("field", [0, 1, 2])
def test_new_fragments_carry_the_rows_and_features_the_lanes_hold(field, golden, states, latents):
    g = golden("g3_decoder")
    st = states["decoder"]
    zs, za = latents
    p, r = torch.from_numpy(g["p_64"][:, :48]), torch.from_numpy(g["r_64"][:, :48])
    pe = O.posenc(p, 10)[0].double().numpy()
    pev = O.posenc(r / torch.norm(r, dim=-1, keepdim=True), 4)[0].double().numpy()
    fi = 1 if field == 1 else 0
    sig = {0: g["sig_aud"][0], 1: g["sig_torso"][0], 2: None}[field]
    made = []

    def reader(flat):
        made.append(BothReaders(field, flat))
        return made[-1]
    feat, sigma = tpp.emulate(1, field, st, pe, pev, None if sig is None else sig.astype(np.float64),
                              zs[0, fi].astype(np.float64), za[0, fi].astype(np.float64), reader=reader)
    rd = made[0]
    assert rd.groups > 40 and (rd.new.plan[rd.new.frag * 512:] == -1).all()          # the whole stream was walked
    name = {0: "head", 1: "torso", 2: "listener"}[field]
    np.testing.assert_allclose(feat, g[f"feat_{name}_64"][0, :48], atol=2e-5, rtol=0)        # test_plan_reproduces_reference_decoder's
    np.testing.assert_allclose(sigma, g[f"sigma_{name}_64"][0, :48], atol=2e-4, rtol=1e-5)


def test_operand_octets_match_the_stream_slots_and_the_bias_vectors():
    """k-group g's eight features of a tile are, in order, k-slot (k-unit g >> 1, half g & 1) of the 32x32x16 map - what makes one
    whole stream slot the A operand - and the lane's bias octet holds the biases of exactly those rows ([tile][half][16] floats)."""
    for lane in range(64):
        g = lane >> 4
        want = [tpp.kslot_to_slot(1, g >> 1, g & 1, e) for e in range(8)]
        assert M["feat"][lane].tolist() == want
        b = int(M["bias"][lane])
        assert b % 8 == 0 and [tpp.tile_feat((b + e) >> 4, (b + e) & 15) for e in range(8)] == want
    # the accumulator rows of (T, j): MFMA row 4 g + j of half T is the tile row the operand octet names at e = 4 T + j
    for g in range(4):
        for T in range(2):
            for j in range(4):
                assert m16_row(4 * g + j, T) == M["feat"][16 * g][4 * T + j]


def test_dma_permutation_is_a_bijection_per_piece():
    assert sorted(M["dma"].tolist()) == [16 * k for k in range(64)]


def test_every_k_group_reads_256_contiguous_bytes():
    for rd in list(M["rd2"]) + list(M["rd1"]):
        for g in range(4):
            off = np.sort(rd[16 * g:16 * g + 16])
            assert (np.diff(off) == 16).all(), (g, off)
    # tile 1 of a pair is the next fragment, T1 a fixed distance behind T0, k-groups 2, 3 one k-unit (G fragments) behind 0, 1
    assert (M["rd2"][2] - M["rd2"][0] == 1024).all() and (M["rd2"][3] - M["rd2"][1] == 1024).all()
    assert len(set((M["rd2"][1] - M["rd2"][0]).tolist())) == 1 and ((M["rd1"][1] - M["rd1"][0]) == (M["rd2"][1] - M["rd2"][0])).all()
    assert (M["rd2"][0][32:] - M["rd2"][0][:32] == 2048).all() and (M["rd1"][0][32:] - M["rd1"][0][:32] == 1024).all()
