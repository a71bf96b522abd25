"""The f16 tier's renders, bit for bit, against fixtures written ONCE (tests/golden/f16_bits/, by tools/f16_bits_dump.py with the
library of the commit before LABNOTES.md 4.8): performance work on the f16 render kernels may reorder instructions, never results.

Per case float32 rgb_head / rgb_com, the per-sample weights and the depths of 20 consecutive rays (f16: three workgroups of eight
waves, the last one with four live waves), for two windows stacked on axis 0 of every fixture:
  window 0: rays 101,250 .. 101,269 of the 450 x 450 synthetic scene (row 225 from the left edge: mostly empty space);
  window 1: the 20 rays of the same row across the middle of the head (a pin on empty space alone would pin only the background
            sample's weight).
Cases: sample counts 64+0, 32+32 and 64+128; one and two fields; the 256-wide decoder (two fields: the blend decoder of
tests/blend_scene.py, on which both fields carry weight) and a 128-wide one on the native 128-wide program.

The same fixtures are asserted through the entry points that equal the plain launch by the project's own tests: supplied pinhole
rays (test_gpu_rays), supplied depths where n_fine == 0 (test_gpu_zvals) and the rgb of the aux launch (test_gpu_aux)."""
import os

import numpy as np
import pytest
import torch

import blend_scene as B
from dfanerf import synth

pytestmark = pytest.mark.gpu
t = torch.from_numpy
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "f16_bits")
N = 20
FRAME = B.FRAME
WINDOWS = (101250, 225 * 450 + 215)
COUNTS = ((64, 0), (32, 32), (64, 128))
CASES = [(w, f, nc, nf) for w in (256, 128) for f in (1, 2) for nc, nf in COUNTS]
NAMES = ("rgb_head", "rgb_com", "w_head", "w_com", "z")


def case_name(width, fields, nc, nf):
    return f"w{width}_f{fields}_{nc}p{nf}"


def fixture_path(case, name):
    return os.path.join(FIX, f"{case_name(*case)}_{name}.npy")


class World:
    """everything the launches of every case share, built once: scene, background, pinhole rays, packed decoders and biases"""

    def __init__(self, eng, scene, states, latents, golden):
        self.eng, self.scene = eng, scene
        assert scene["H"] == 450 and scene["W"] == 450
        self.bg = (t(scene["bg"]).float() / 255.0).reshape(-1, 3).cuda()
        geo = (scene["H"], scene["W"], scene["focal"])
        o_h, d_h = eng.get_rays(*geo, scene["poses"][FRAME], scene["cx"], scene["cy"])
        o_t, d_t = eng.get_rays(*geo, scene["pose_body"], scene["cx"], scene["cy"])
        self.rays4 = [x.reshape(-1, 3) for x in (o_h, d_h, o_t, d_t)]
        g7, g3 = golden("g7_frame_coarse"), golden("g3_decoder")
        zs, za = synth.synth_latents(0, z_dim=64)
        self.cond = {256: B.conditioning(g7, latents), 128: (g3["sig_aud"][0], g3["sig_torso"][0], zs[0], za[0])}
        self.state = {(256, 1): states["decoder"], (256, 2): B.blend_state(states),
                      (128, 1): synth.synth_decoder_state(0, z_dim=64, hidden=128)}
        self.state[(128, 2)] = self.state[(128, 1)]
        self._pk = {}

    def packed(self, width, fields):
        key = (width, 2 if (width, fields) == (256, 2) else 1)
        if key not in self._pk:
            flat = self.eng.flatten_state(self.state[(width, fields)], "cuda")
            kw = {} if width == 256 else {"z_dim": 64, "width": 128}
            self._pk[key] = self.eng.PackedDecoder(flat, "f16", fields=(0, 1), **kw)
        pk = self._pk[key]
        sa, stt, zs, za = self.cond[width]
        return pk, pk.fold(sa, stt if fields == 2 else None, zs, za)

    def frame(self, begin, nc, nf, fields):
        sc = self.scene
        return self.eng.make_frame(sc["H"], sc["W"], sc["focal"], sc["cx"], sc["cy"], sc["poses"][FRAME], sc["pose_body"], sc["near"],
                                   sc["far"], ray_begin=begin, ray_count=N, n_coarse=nc, n_fine=nf, fields=fields)

    def plain(self, case, begin):
        """the plain launch of one window -> {name: float32 cpu tensor} (the com entries missing with one field)"""
        width, fields, nc, nf = case
        pk, bias = self.packed(width, fields)
        out = self.eng.render(pk, bias, self.frame(begin, nc, nf, fields), self.bg, want_weights=True, want_z=True)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in zip(NAMES, out) if v is not None}

    def through(self, case, begin, route, z=None):
        """the same rays through another entry point -> {name: tensor} of what that entry point returns"""
        width, fields, nc, nf = case
        pk, bias = self.packed(width, fields)
        fr = self.frame(begin, nc, nf, fields)
        if route == "rays":
            sel = torch.arange(begin, begin + N, device="cuda")
            r4 = [x[sel].contiguous() for x in self.rays4]
            rays = self.eng.pack_rays(r4[0], r4[1], *(r4[2:] if fields == 2 else ()))
            out = self.eng.render(pk, bias, fr, self.bg[sel].contiguous(), rays=rays, want_weights=True, want_z=True)
            names = NAMES
        elif route == "z":
            out = self.eng.render(pk, bias, fr, self.bg, want_weights=True, want_z=True, z_vals=z.cuda())
            names = NAMES
        else:
            out = self.eng.render(pk, bias, fr, self.bg, want_aux=True)[:2]
            names = NAMES[:2]
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in zip(names, out) if v is not None}


@pytest.fixture(scope="module")
def world(scene, states, latents, golden):
    from dfanerf import engine
    engine.require_gpu()
    return World(engine, scene, states, latents, golden)


def _same(got, want, what):
    assert set(got) <= set(want), what
    for k, a in got.items():
        b = want[k]
        assert a.dtype == torch.float32 and a.shape == b.shape and torch.equal(a, b), \
            (what, k, float((a - b).abs().max()), int((a != b).sum()))


@pytest.mark.parametrize("width,fields,nc,nf", CASES, ids=[case_name(*c) for c in CASES])
def test_f16_render_bits(world, width, fields, nc, nf):
    case = (width, fields, nc, nf)
    want = {k: t(np.load(fixture_path(case, k))) for k in NAMES if fields == 2 or not k.endswith("_com")}
    assert want["z"].shape == (len(WINDOWS), N, nc + nf) and want["rgb_head"].shape == (len(WINDOWS), N, 3)
    # the fixtures are no pin on empty space: in the middle window some ray leaves a tenth of its weight or more in front of the
    # background sample (0.32 with the translucent blend decoder, 0.97 and more with the others), and the pixels differ
    assert float(want["w_head"][1, :, :-1].sum(1).max()) > 0.1 and float(want["rgb_head"][1].std()) > 0.01
    for wi, begin in enumerate(WINDOWS):
        fix = {k: v[wi] for k, v in want.items()}
        got = world.plain(case, begin)
        assert set(got) == set(fix)
        _same(got, fix, (case, begin, "plain"))
        _same(world.through(case, begin, "rays"), fix, (case, begin, "rays"))
        _same(world.through(case, begin, "aux"), fix, (case, begin, "aux"))
        if nf == 0:
            _same(world.through(case, begin, "z", fix["z"]), fix, (case, begin, "z"))
