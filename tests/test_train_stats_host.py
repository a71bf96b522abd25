"""Host-side checks (no GPU) of the training step's opacity / expected depth: dfn_composite_stats and dfn_composite_bwd_stats are
declared and bound, refuse what include/dfanerf.h says they refuse - before any device work, with the rule in the message - and the
scene the GPU tests (tests/test_gpu_train_stats.py) hold the step against is not vacuous for a matte or depth loss."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import blend_scene as B
import train_stats_ref as R
from dfanerf import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "dfanerf.h")
ONE = C.c_void_p(16)          # a non-null address that is never dereferenced: every call below returns before it would be
ODD = C.c_void_p(20)          # ... and one that is not 16-byte aligned


def _frame(nc, nf, fields=2, rays=8):
    fr = _lib.DfnFrame()
    fr.ray_count, fr.n_coarse, fr.n_fine, fr.fields, fr.concate_bg, fr.H, fr.W = rays, nc, nf, fields, 1, 4, 4
    return fr


def _stats(fr, pix=ONE, rays=None, bounds=None, samples=ONE, z_all=None, ranks=None, stats=ONE):
    return _lib.lib.dfn_composite_stats(C.byref(fr) if fr is not None else None, pix, rays, bounds, samples, z_all, ranks, stats, None)


def _bwd(fr, pix=ONE, rays=None, bounds=None, bg_f32=ONE, bg_u8=None, samples=ONE, z_all=None, ranks=None, d_h=ONE, d_c=ONE, d_s=ONE,
         dsamples=ONE, zero_buf=None, zero_n=0, d_norm=None):
    return _lib.lib.dfn_composite_bwd_stats(C.byref(fr) if fr is not None else None, pix, rays, bounds, bg_f32, bg_u8, samples, z_all, ranks,
                                            d_h, d_c, d_s, dsamples, zero_buf, zero_n, d_norm, None)


def _refused(rc, text):
    msg = _lib.lib.dfn_last_error()
    assert rc == -1 and text in msg, (rc, msg)


# ---- 1. binding ----------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_and_the_library_binds_both_entry_points():
    src = open(HEADER).read()
    for name in ("dfn_composite_stats", "dfn_composite_bwd_stats"):
        assert re.search(r"^int %s\(const DfnFrame\* frame, const int32_t\* pix_index, const float\* rays, const float\* bounds," % name, src,
                         re.M), name
        assert name in _lib.EXPORTS and getattr(_lib.lib, name).restype is C.c_int
    # each cites the reference's weights and composite: MAIN:169-179 / 146-166
    for name in ("dfn_composite_stats", "dfn_composite_bwd_stats"):
        doc = src[:src.index("int %s(" % name)].rsplit("*/", 2)[-2]
        assert "MAIN:169-179" in doc and "146-166" in doc, name
    assert len(_lib.lib.dfn_composite_stats.argtypes) == 9 and len(_lib.lib.dfn_composite_bwd_stats.argtypes) == 17


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------
def test_null_pointers():
    fr = _frame(64, 0)
    _refused(_stats(None), b"dfn_composite_stats: a NULL pointer")
    _refused(_stats(fr, samples=None), b"dfn_composite_stats: a NULL pointer")
    _refused(_stats(fr, stats=None), b"dfn_composite_stats: a NULL pointer")
    _refused(_bwd(None), b"dfn_composite_bwd_stats: a NULL pointer")
    for k in ("samples", "d_h", "d_c", "d_s", "dsamples"):
        _refused(_bwd(fr, **{k: None}), b"dfn_composite_bwd_stats: a NULL pointer")
    _refused(_bwd(fr, bg_f32=None), b"dfn_composite_bwd_stats: no background given")
    assert _bwd(_frame(64, 0, rays=0), bg_f32=None, bg_u8=ONE) == 0


@pytest.mark.parametrize("call,who", [(_stats, b"dfn_composite_stats"), (_bwd, b"dfn_composite_bwd_stats")])
def test_the_shared_refusals(call, who):
    fr = _frame(64, 0)
    _refused(call(fr, pix=ONE, rays=ONE), who + b": exactly one of pix_index / rays selects the ray source (both given)")
    _refused(call(fr, pix=None, rays=None), who + b": exactly one of pix_index / rays selects the ray source (neither given)")
    _refused(call(fr, pix=ONE, bounds=ONE), who + b": bounds are the per-ray (near, far) of caller-supplied rays")
    for rays in (None, ONE):
        src = dict(pix=None, rays=ONE, bounds=ONE) if rays else dict(pix=ONE)
        _refused(call(_frame(64, 0, fields=1), **src), who + b": the training step renders two fields")
        for nc, nf in ((48, 0), (96, 0), (32, 32), (32, 64), (64, 32), (64, 96), (128, 64), (32, 128)):
            _refused(call(_frame(nc, nf), z_all=ONE, ranks=ONE, **src), who + b": 32, 64 or 128 coarse samples, or 64 coarse + 64 or 128 fine")
            # ... before the empty-launch shortcut
            _refused(call(_frame(nc, nf, rays=0), z_all=ONE, ranks=ONE, **src), who + b": 32, 64 or 128 coarse samples")
        for nf in (64, 128):
            _refused(call(_frame(64, nf), **src), who + b": the hierarchical step (n_fine > 0) needs z_all and ranks")
            _refused(call(_frame(64, nf), z_all=ONE, **src), who + b": the hierarchical step (n_fine > 0) needs z_all and ranks")
            _refused(call(_frame(64, nf), ranks=ONE, **src), who + b": the hierarchical step (n_fine > 0) needs z_all and ranks")


def test_the_backwards_own_refusals():
    fr = _frame(64, 0)
    _refused(_bwd(fr, zero_buf=ODD, zero_n=64), b"dfn_composite_bwd_stats: zero_buf must be 16-byte aligned")
    _refused(_bwd(fr, pix=None, rays=ONE, zero_buf=ODD, zero_n=64), b"dfn_composite_bwd_stats: zero_buf must be 16-byte aligned")
    _refused(_bwd(fr, zero_buf=ONE, zero_n=-4), b"dfn_composite_bwd_stats: zero_buf must be 16-byte aligned")
    _refused(_bwd(fr, d_norm=ONE), b"dfn_composite_bwd_stats: d_norm is the gradient of the norms of caller-supplied rays (rays is NULL)")


@pytest.mark.parametrize("nc,nf", R.CONFIGS)
def test_an_empty_launch_returns_ok(nc, nf):
    hier = dict(z_all=ONE, ranks=ONE) if nf else {}
    fr = _frame(nc, nf, rays=0)
    for src in (dict(pix=ONE), dict(pix=None, rays=ONE), dict(pix=None, rays=ONE, bounds=ONE)):
        assert _stats(fr, **hier, **src) == 0, _lib.lib.dfn_last_error()
        assert _bwd(fr, **hier, **src) == 0, _lib.lib.dfn_last_error()
        assert _bwd(fr, zero_buf=ONE, zero_n=64, **hier, **src) == 0, _lib.lib.dfn_last_error()
    assert _bwd(fr, pix=None, rays=ONE, d_norm=ONE, **hier) == 0, _lib.lib.dfn_last_error()


def test_the_existing_family_keeps_its_messages():
    """the entry points the new one stands in for are untouched: the same checks, the same words"""
    L = _lib.lib
    fr = _frame(32, 32)
    assert L.dfn_composite_bwd_hier_z(C.byref(fr), ONE, ONE, None, ONE, ONE, ONE, ONE, ONE, ONE, None, 0, None) == -1
    assert b"dfn_composite_bwd_hier: 64 coarse + 64 or 128 fine samples" in L.dfn_last_error()
    fr = _frame(64, 0)
    assert L.dfn_composite_bwd_rays_zg(C.byref(fr), ONE, None, ONE, None, ONE, ONE, ONE, ONE, None, 0, None, None) == -1
    assert b"dfn_composite_bwd_rays_zg: d_norm is NULL" in L.dfn_last_error()
    assert L.dfn_composite_bwd_z(C.byref(fr), ONE, ONE, None, ONE, ONE, ONE, ONE, ODD, 4, None) == -1
    assert b"dfn_composite_bwd_z: zero_buf must be 16-byte aligned" in L.dfn_last_error()


def test_render_train_refuses_stats_without_a_ray_source():
    from dfanerf import training
    with pytest.raises(ValueError, match="want_stats needs pix_index or rays"):
        training.render_train(None, None, _frame(64, 0), None, None, None, None, None, None, want_stats=True)


# ---- 3. the oracle scene is not vacuous ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orc(scene, states, latents, golden):
    return B.Oracle(scene, B.blend_state(states), latents, golden("g7_frame_coarse"), pix=B.ray_indices(scene, R.N_RAYS))


def _figures(orc, nc, nf):
    aux = orc.render(nc, nf, 2)[2]
    z = (aux["z_all"] if nf else aux["z_coarse"]).contiguous()
    s_h, f_h, s_t, f_t = orc.fields_at(z.numpy(), 2)
    s_h, s_t = s_h.clone().requires_grad_(True), s_t.clone().requires_grad_(True)
    rh, wh, rc, wc = orc.integrate(z.numpy(), s_h, f_h, s_t, f_t)
    stats = R.stats_of(wh, wc, z)
    tgt = torch.rand(len(orc.pix), 3, generator=torch.Generator().manual_seed(5))
    g_s = torch.autograd.grad(R.stats_loss(stats, R.matte(len(orc.pix))), (s_h, s_t), retain_graph=True)
    g_c = torch.autograd.grad(R.colour_loss(rh, rc, tgt), (s_h, s_t))
    norm = lambda g: float(torch.cat([x.reshape(-1) for x in g]).double().norm())
    return stats.detach().numpy(), norm(g_s), norm(g_c)


@pytest.mark.parametrize("nc,nf", R.CONFIGS)
def test_the_oracle_scene_is_not_vacuous_for_a_stats_loss(orc, nc, nf):
    """conditions, not measurements: on the blend decoder most rays are translucent in the composite, a good share in the head image,
    and the stats loss moves the raw densities at least as much as the colour loss does.  (With the oracle: 100 % of the rays have
    acc_com in (0.05, 0.95), 35 - 46 % acc_head; the gradient ratio is 6.6 - 8.4.)"""
    stats, g_s, g_c = _figures(orc, nc, nf)
    mid = lambda a: float(((a > 0.05) & (a < 0.95)).mean())
    print(f"{nc} + {nf}: acc_com in (0.05, 0.95) on {100 * mid(stats[:, 2]):.0f} % of the rays (range {stats[:, 2].min():.2f} - "
          f"{stats[:, 2].max():.2f}), acc_head on {100 * mid(stats[:, 0]):.0f} %; |d stats loss / d sigma| / |d colour loss / d sigma| = "
          f"{g_s / g_c:.1f}")
    assert stats.shape == (R.N_RAYS, 4) and np.isfinite(stats).all()
    assert mid(stats[:, 2]) >= 0.9
    assert mid(stats[:, 0]) >= 0.3
    assert g_s >= g_c > 0
    # depth is premultiplied: between near * acc and far * acc
    for a, d in ((0, 1), (2, 3)):
        assert (stats[:, d] >= orc.near * stats[:, a] - 1e-5).all() and (stats[:, d] <= orc.far * stats[:, a] + 1e-5).all()


def test_the_fixtures_decoder_would_fail_the_condition(scene, states, latents, golden):
    o = B.Oracle(scene, states["decoder"], latents, golden("g7_frame_coarse"), pix=B.ray_indices(scene, R.N_RAYS))
    stats, _, _ = _figures(o, 64, 0)
    assert (stats[:, 2] > 0.999).all()


def test_the_ordered_sum_is_a_sum():
    """the numpy restatement of the kernel's summation order against float64, and its lane ownership: K consecutive positions a lane"""
    rs = np.random.RandomState(0)
    for S, K in ((32, 1), (64, 1), (128, 2), (192, 3)):
        w, z = rs.rand(5, S).astype(np.float32) / S, np.sort(rs.uniform(0.3, 0.9, (5, S)).astype(np.float32), 1)
        for cbg in (True, False):
            fg = slice(0, S - 1) if cbg else slice(None)
            a, d = R.ordered_sums(w, z, K, cbg)
            assert a.dtype == np.float32 and d.dtype == np.float32
            np.testing.assert_allclose(a, w[:, fg].astype(np.float64).sum(1), rtol=0, atol=S * 2.0 ** -24)
            np.testing.assert_allclose(d, (w[:, fg].astype(np.float64) * z[:, fg]).sum(1), rtol=0, atol=S * 2.0 ** -24)
