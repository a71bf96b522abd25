"""Every render variant of csrc/dfn_render_variants.h launched once through its public entry points, at the smallest shape that still
exercises the dispatch: an 8 x 8 image = 64 rays, 32 coarse samples; n_fine = 0 always and 32 where the variant has a fine pass;
two fields always and one where the variant renders (the training step is two fields).

Every output an entry point promises is pre-filled with a sentinel - NaN for floats, 0xFF bytes for uint8 / uint16 - and must hold
none after the launch; what the form does not write (the inputs that ride in output slots of the argument block: bounds, zvals) must be
untouched.  The scene is chosen so that 0xFF is no value the kernels produce in an image: the background is at most 0.5, so no colour
reaches 1.0 (to8b truncates: 255 needs exactly 1.0; asserted on the f32 form).  The composite's OPACITY is exactly 1.0 - it ends on the
background plane - so alpha8_com is 255 by right: the u8 aux form is launched on two fills, 0xFF and 0x00, and the results must agree
(a byte that was not written keeps its fill).  The recorder's act_T and masks have
structural padding the recorder never writes, and all-ones is a valid code and a valid mask word: for them the test asserts that the
fill is gone, and bit equality with the plain step where there is one to compare with.

Where the suite asserts bit equality between forms at its own shapes, the same holds here: pinhole rays = the plain launch, a z launch
fed the plain launch's depths = the plain launch, the training step on pinhole rays = the plain step.

The cases are looked up by the variant's flags as parsed from the header: a new line there without a case here fails."""
import ctypes as C

import pytest
import torch

import blend_scene as B
from dfanerf import _lib, synth
from test_variant_list_host import TIERS, VARIANTS

pytestmark = pytest.mark.gpu

L = _lib.lib
HW, N, NC = 8, 64, 32
TIER_NAME = {"TIER_F32": "f32", "TIER_BF16": "bf16", "TIER_F16": "f16", "TIER_F16X3": "f16x3"}
FRAME = 2


@pytest.fixture(scope="module")
def eng():
    from dfanerf import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope="module")
def nets(eng, states, golden, latents):
    """width -> (flat parameters, conditioning, z_dim): the fixtures' synthetic decoder, and its 128-wide sibling (tests/test_gpu_narrow.py)"""
    g3 = golden("g3_decoder")
    zs, za = synth.synth_latents(0, z_dim=64)
    return {256: (eng.flatten_state(states["decoder"], "cuda"), B.conditioning(golden("g7_frame_coarse"), latents), 256),
            128: (eng.flatten_state(synth.synth_decoder_state(0, z_dim=64, hidden=128), "cuda"),
                  (g3["sig_aud"][0], g3["sig_torso"][0], zs[0], za[0]), 64)}


@pytest.fixture(scope="module")
def packed(eng, nets):
    cache = {}

    def get(tier, width, fields):
        """-> (PackedDecoder, folded bias) of this tier and width for a one- or two-field launch"""
        flat, (sa, stt, zs, za), z_dim = nets[width]
        if (tier, width) not in cache:
            cache[tier, width] = eng.PackedDecoder(flat, tier, z_dim=z_dim, width=width)
        if (tier, width, fields) not in cache:
            cache[tier, width, fields] = cache[tier, width].fold(sa, stt if fields == 2 else None, zs, za)
        return cache[tier, width], cache[tier, width, fields]
    return get


@pytest.fixture(scope="module")
def bg():
    return (torch.rand(N, 3, generator=torch.Generator().manual_seed(1)) * 0.5).cuda()


def _frame(eng, scene, n_fine, fields):
    k = HW / scene["W"]
    return eng.make_frame(HW, HW, scene["focal"] * k, HW / 2, HW / 2, scene["poses"][FRAME], scene["pose_body"], scene["near"], scene["far"],
                          ray_begin=0, ray_count=N, n_coarse=NC, n_fine=n_fine, fields=fields)


def _pinhole_rays(eng, scene, fields):
    k = HW / scene["W"]
    geo = (HW, HW, scene["focal"] * k)
    parts = eng.get_rays(*geo, scene["poses"][FRAME], HW / 2, HW / 2)
    if fields == 2:
        parts += eng.get_rays(*geo, scene["pose_body"], HW / 2, HW / 2)
    return eng.pack_rays(*(x.reshape(-1, 3) for x in parts))


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _ff(n_bytes, fill=0xFF):
    return torch.full((int(n_bytes),), fill, dtype=torch.uint8, device="cuda")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _net(pk, bias, fr, tier_arg=None):
    two = fr.fields == 2
    bias_t = C.c_void_p(bias.data_ptr() + 4 * pk.bias_floats(0)) if two else None
    return (pk.tier_arg if tier_arg is None else tier_arg, C.byref(fr), _p(pk.packed[0]), _p(pk.packed[1]) if two else None, _p(bias), bias_t)


def _done(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, (what, L.dfn_last_error())


def _no_nan(what, **outs):
    for k, v in outs.items():
        assert bool(torch.isfinite(v).all()), (what, k, "sentinel left")


def _no_ff(what, **outs):
    for k, v in outs.items():
        b = v.view(torch.uint8).reshape(v.shape[0], -1)
        assert not bool((b == 0xFF).all(dim=1).any()), (what, k, "sentinel left")


# ---- the launches: each fills its outputs with the sentinel, launches, checks the promised ones, returns them ------------------------
def render_f32(name, pk, bias, fr, bg, rays=None, bounds=None, zvals=None):
    two, S = fr.fields == 2, fr.n_coarse + fr.n_fine
    o = dict(rgb_head=_nan(N, 3), w_head=_nan(N, S), z=_nan(N, S))
    if two:
        o.update(rgb_com=_nan(N, 3), w_com=_nan(N, S))
    outs = (_p(o["rgb_head"]), _p(o.get("rgb_com")), _p(o["w_head"]), _p(o.get("w_com")), _p(o["z"]))
    ins = [x if x is None else x.clone() for x in (rays, bounds, zvals)]
    if name == "dfn_render_rays_fwd":
        rc = L.dfn_render_rays_fwd(*_net(pk, bias, fr), _p(rays), _p(bounds), _p(bg), None, *outs, None)
    elif name == "dfn_render_z_fwd":
        rc = L.dfn_render_z_fwd(*_net(pk, bias, fr), _p(bg), None, None, *outs, _p(zvals), None)
    else:
        rc = L.dfn_render_fwd(*_net(pk, bias, fr), _p(bg), None, None, *outs, None)
    _done(rc, name)
    _no_nan((name, fr.fields, fr.n_fine), **o)
    for was, now in zip(ins, (rays, bounds, zvals)):        # inputs in output slots: read, never written
        assert was is None or torch.equal(was, now), name
    assert float(o["rgb_head"].max()) < 1.0 and float(o["rgb_head"].std()) > 0
    return o


def render_u8(name, pk, bias, fr, bg, rays=None, bounds=None, zvals=None):
    two = fr.fields == 2
    o = dict(rgb8_head=_ff(N * 3).view(N, 3))
    if two:
        o.update(rgb8_com=_ff(N * 3).view(N, 3))
    outs = (_p(o["rgb8_head"]), _p(o.get("rgb8_com")))
    if name == "dfn_render_rays_fwd_u8":
        rc = L.dfn_render_rays_fwd_u8(*_net(pk, bias, fr), _p(rays), _p(bounds), _p(bg), None, *outs, None)
    elif name == "dfn_render_z_fwd_u8":
        rc = L.dfn_render_z_fwd_u8(*_net(pk, bias, fr), _p(bg), None, None, *outs, _p(zvals), None)
    else:
        rc = L.dfn_render_fwd_u8(*_net(pk, bias, fr), _p(bg), None, None, *outs, None)
    _done(rc, name)
    for k, v in o.items():
        assert not bool((v == 0xFF).any()), (name, k, "sentinel left")
    return o


def render_aux(pk, bias, fr, bg):
    two = fr.fields == 2
    o = dict(rgb_head=_nan(N, 3), aux_head=_nan(N, 2))
    if two:
        o.update(rgb_com=_nan(N, 3), aux_com=_nan(N, 2))
    _done(L.dfn_render_fwd_aux(*_net(pk, bias, fr), _p(bg), None, None, _p(o["rgb_head"]), _p(o.get("rgb_com")), _p(o["aux_head"]),
                               _p(o.get("aux_com")), None), "dfn_render_fwd_aux")
    _no_nan(("dfn_render_fwd_aux", fr.fields, fr.n_fine), **o)
    # the u8 form.  The composite image ends on the background plane: its opacity is exactly 1.0, alpha8_com = 255 = the sentinel.
    # So this form is launched on two fills, 0xFF and 0x00: a byte the kernel did not write keeps its fill and differs
    def launch(fill):
        u = dict(rgb8_head=_ff(N * 3, fill).view(N, 3), alpha8_head=_ff(N, fill), depth16_head=_ff(2 * N, fill).view(N, 2))
        if two:
            u.update(rgb8_com=_ff(N * 3, fill).view(N, 3), alpha8_com=_ff(N, fill), depth16_com=_ff(2 * N, fill).view(N, 2))
        _done(L.dfn_render_fwd_u8_aux(*_net(pk, bias, fr), _p(bg), None, None, _p(u["rgb8_head"]), _p(u.get("rgb8_com")), _p(u["alpha8_head"]),
                                      _p(u.get("alpha8_com")), _p(u["depth16_head"]), _p(u.get("depth16_com")), None), "dfn_render_fwd_u8_aux")
        return u
    u = launch(0xFF)
    _same(u, launch(0x00), ("dfn_render_fwd_u8_aux", fr.fields, fr.n_fine, "a byte was not written"))
    for k, v in u.items():
        if k.startswith("rgb8"):
            assert not bool((v == 0xFF).any()), ("dfn_render_fwd_u8_aux", k, "sentinel left")
        elif k.startswith("depth16"):
            _no_ff("dfn_render_fwd_u8_aux", **{k: v})
    for img in ("head", "com")[:fr.fields]:              # (255 is to8b of opacity 1.0 exactly, as the f32 form of this tier reports it)
        assert not bool(((u["alpha8_" + img] == 0xFF) & (o["aux_" + img][:, 0] < 1.0)).any()), ("alpha8_" + img, "sentinel left")


def train_fwd(name, tier_arg, pk, bias, fr, bg, rays=None, bounds=None):
    """one training forward; name: dfn_train_fwd[_hier][_loss] or dfn_train_rays_fwd[_hier]"""
    hier, S = fr.n_fine > 0, fr.n_coarse + fr.n_fine
    NP = N * S
    rows = lambda f, w: _lib.check(L.dfn_train_rows(f, w), "dfn_train_rows")
    tier = tier_arg & 0xFF
    act_sel = 8 if tier_arg & _lib.TRAIN_ACT_E4M3 else 6
    o = dict(rgb_head=_nan(N, 3), rgb_com=_nan(N, 3), samples=_nan(NP, 8))
    for f in (0, 1):
        o["act%d" % f] = _ff(rows(f, 0) * NP * 4 if tier == _lib.TIER_F32 else (NP // 32 + 1) * rows(f, act_sel))
        o["masks%d" % f] = _ff(NP // 32 * rows(f, 2) * 64 * 4)
    rec = (_p(o["rgb_head"]), _p(o["rgb_com"]), _p(o["samples"]), _p(o["act0"]), _p(o["masks0"]), _p(o["act1"]), _p(o["masks1"]))
    if hier:
        o.update(z_all=_nan(N, S), ranks=_ff(N * S).view(N, S))
    extra = (_p(o["z_all"]), _p(o["ranks"])) if hier else ()
    net = _net(pk, bias, fr, tier_arg)
    pix = torch.arange(N, dtype=torch.int32, device="cuda")
    if rays is not None:
        was = bounds.clone()
        rc = getattr(L, name)(*net, _p(rays), _p(bounds), _p(bg), None, *rec, *extra, None)
    elif name.endswith("_loss"):
        img = torch.randint(0, 256, (2, N, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
        ws = torch.zeros(_lib.check(L.dfn_train_loss_floats(N), "dfn_train_loss_floats"), dtype=torch.float32, device="cuda")
        o.update(d_rgb_head=_nan(N, 3), d_rgb_com=_nan(N, 3), losses=_nan(3))
        loss = _lib.DfnTrainLoss(img[0].data_ptr(), img[1].data_ptr(), o["d_rgb_head"].data_ptr(), o["d_rgb_com"].data_ptr(),
                                 o["losses"].data_ptr(), ws.data_ptr())
        rc = getattr(L, name)(*net, _p(bg), None, _p(pix), *rec, *extra, C.byref(loss), None)
    else:
        rc = getattr(L, name)(*net, _p(bg), None, _p(pix), *rec, *extra, None)
    _done(rc, name)
    what = (name, hex(tier_arg), fr.n_fine)
    _no_nan(what, **{k: v for k, v in o.items() if v.dtype == torch.float32})
    for f in (0, 1):
        assert bool((o["act%d" % f] != 0xFF).any()) and bool((o["masks%d" % f] != 0xFF).any()), (what, f, "recorder wrote nothing")
        if act_sel == 8:        # the e4m3 recorder's tiles are twice the fp4 recorder's: the fp4 kernels in its place would stop short
            assert bool((o["act%d" % f][NP // 32 * rows(f, 6):NP // 32 * rows(f, 8)] != 0xFF).any()), (what, f, "not the e4m3 recorder")
    if hier:
        assert int(o["ranks"].max()) < S, what
    if rays is not None:
        assert torch.equal(was, bounds), (what, "bounds ride in the head weights' slot: read, never written")
    return o


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


# ---- one case per set of flags (TIER_W128 aside: it selects the network) ---------------------------------------------------------------
def case_plain(eng, scene, packed, bg, tier, width):
    for fields in (2, 1):
        pk, bias = packed(tier, width, fields)
        for n_fine in (0, 32):
            fr = _frame(eng, scene, n_fine, fields)
            render_f32("dfn_render_fwd", pk, bias, fr, bg)
            render_u8("dfn_render_fwd_u8", pk, bias, fr, bg)
    if tier in ("f32", "bf16") and width == 256:           # a trainable tier's unit also holds the training forwards (recorder on)
        pk, bias = packed(tier, width, 2)
        for n_fine in (0, 32):
            fr = _frame(eng, scene, n_fine, 2)
            name = "dfn_train_fwd_hier" if n_fine else "dfn_train_fwd"
            train_fwd(name, TIERS["TIER_" + tier.upper()], pk, bias, fr, bg)
            train_fwd(name + "_loss", TIERS["TIER_" + tier.upper()], pk, bias, fr, bg)


def case_aux(eng, scene, packed, bg, tier, width):
    for fields in (2, 1):
        pk, bias = packed(tier, width, fields)
        for n_fine in (0, 32):
            render_aux(pk, bias, _frame(eng, scene, n_fine, fields), bg)


def case_rays(eng, scene, packed, bg, tier, width):
    for fields in (2, 1):
        pk, bias = packed(tier, width, fields)
        rays = _pinhole_rays(eng, scene, fields)
        bounds = torch.tensor([scene["near"], scene["far"]], dtype=torch.float32, device="cuda").repeat(N, 1)
        for n_fine in (0, 32):
            fr = _frame(eng, scene, n_fine, fields)
            plain = render_f32("dfn_render_fwd", pk, bias, fr, bg)
            _same(render_f32("dfn_render_rays_fwd", pk, bias, fr, bg, rays=rays), plain, ("rays", tier, width, fields, n_fine))
            _same(render_f32("dfn_render_rays_fwd", pk, bias, fr, bg, rays=rays, bounds=bounds), plain, ("rays + bounds", tier, width, fields))
            _same(render_u8("dfn_render_rays_fwd_u8", pk, bias, fr, bg, rays=rays, bounds=bounds),
                  render_u8("dfn_render_fwd_u8", pk, bias, fr, bg), ("rays u8", tier, width, fields, n_fine))


def case_z(eng, scene, packed, bg, tier, width):
    for fields in (2, 1):               # (no fine pass: the depths come from memory)
        pk, bias = packed(tier, width, fields)
        fr = _frame(eng, scene, 0, fields)
        plain = render_f32("dfn_render_fwd", pk, bias, fr, bg)
        z = plain["z"].clone()
        _same(render_f32("dfn_render_z_fwd", pk, bias, fr, bg, zvals=z), plain, ("z", tier, width, fields))
        _same(render_u8("dfn_render_z_fwd_u8", pk, bias, fr, bg, zvals=z), render_u8("dfn_render_fwd_u8", pk, bias, fr, bg),
              ("z u8", tier, width, fields))


def case_e4m3(eng, scene, packed, bg, tier, width):
    assert tier == "bf16" and width == 256
    pk, bias = packed(tier, width, 2)
    for n_fine in (0, 32):
        train_fwd("dfn_train_fwd_hier" if n_fine else "dfn_train_fwd", _lib.TIER_BF16 | _lib.TRAIN_ACT_E4M3, pk, bias,
                  _frame(eng, scene, n_fine, 2), bg)


def case_train_rays(eng, scene, packed, bg, tier, width, e4m3=False):
    assert tier in ("f32", "bf16") and width == 256
    pk, bias = packed(tier, width, 2)
    tier_arg = TIERS["TIER_" + tier.upper()] | (_lib.TRAIN_ACT_E4M3 if e4m3 else 0)
    rays = _pinhole_rays(eng, scene, 2)
    bounds = torch.tensor([scene["near"], scene["far"]], dtype=torch.float32, device="cuda").repeat(N, 1)
    for n_fine in (0, 32):
        fr = _frame(eng, scene, n_fine, 2)
        hier = "_hier" if n_fine else ""
        plain = train_fwd("dfn_train_fwd" + hier, tier_arg, pk, bias, fr, bg)
        got = train_fwd("dfn_train_rays_fwd" + hier, tier_arg, pk, bias, fr, bg, rays=rays, bounds=bounds)
        _same(got, plain, ("train rays", tier, e4m3, n_fine))


CASES = {frozenset(): case_plain, frozenset(["TIER_AUX"]): case_aux, frozenset(["TIER_RAYS"]): case_rays,
         frozenset(["TIER_ZVALS"]): case_z, frozenset(["TIER_E4M3"]): case_e4m3,
         frozenset(["TIER_RAYS", "TIER_TRAIN"]): case_train_rays,
         frozenset(["TIER_RAYS", "TIER_TRAIN", "TIER_E4M3"]): lambda *a: case_train_rays(*a, e4m3=True)}


@pytest.mark.parametrize("name,tier,flags", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_every_variant_launches_and_writes_what_it_promises(eng, scene, packed, bg, name, tier, flags):
    form = flags - {"TIER_W128"}
    assert form in CASES, f"variant {name}: no case for the flags {sorted(flags)} - add one"
    CASES[form](eng, scene, packed, bg, TIER_NAME[tier], 128 if "TIER_W128" in flags else 256)
