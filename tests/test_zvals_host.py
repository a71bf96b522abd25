"""Host-side checks of rendering at caller-supplied depths (dfn_render_z_fwd, dfn_render_z_fwd_u8) and of the stand-alone fine sampler
(dfn_fine_depths), no GPU: the C ABI and its ctypes binding agree, the entry points' own count rule (n_fine == 0, n_coarse a multiple
of 32 in 32 ... 192) and their refusals hold before any HIP call, the plain entry point keeps its rule, the command line's flag tables
are what they were, and engine.render checks its arguments before it touches a device."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from dfanerf import _lib, engine, run_nerf

ONE = C.c_void_p(16)          # a non-null address that is never dereferenced: every call below returns before it would be
L = _lib.lib
Z_COUNTS = (32, 64, 96, 128, 160, 192)
Z_TIERS = (_lib.TIER_F32, _lib.TIER_F16, _lib.TIER_F16X3)


def _declared_arg_count(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/dfanerf.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def _frame(nc, nf=0, fields=1, rays=8):
    fr = _lib.DfnFrame()
    fr.ray_count, fr.n_coarse, fr.n_fine, fr.fields, fr.concate_bg, fr.H, fr.W = rays, nc, nf, fields, 1, 4, 4
    return fr


def _z_fwd(fr, tier=_lib.TIER_F32, zvals=ONE, bg=ONE, torso=None, bias_t=None, rgb_com=None):
    return L.dfn_render_z_fwd(tier, C.byref(fr), ONE, torso, ONE, bias_t, bg, None, None, ONE, rgb_com, None, None, None, zvals, None)


def _z_fwd_u8(fr, tier=_lib.TIER_F32, zvals=ONE, bg=ONE):
    return L.dfn_render_z_fwd_u8(tier, C.byref(fr), ONE, None, ONE, None, bg, None, None, ONE, None, zvals, None)


def test_header_declares_and_lib_binds_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dfanerf.h")).read()
    for name, n_args in (("dfn_render_z_fwd", 16), ("dfn_render_z_fwd_u8", 13), ("dfn_fine_depths", 4)):
        assert name in _lib.EXPORTS
        assert _declared_arg_count(hdr, name) == len(getattr(L, name).argtypes) == n_args, name
    # the z forms are the plain ones plus `zvals`
    assert _declared_arg_count(hdr, "dfn_render_fwd") == 15 and _declared_arg_count(hdr, "dfn_render_fwd_u8") == 12
    # each declaration cites the reference lines it stands for
    for name, cites in (("dfn_render_z_fwd", ("MAIN:617-619", "MAIN:653-709")), ("dfn_fine_depths", ("HELP:537-581",))):
        comment = hdr[:hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        for c in cites:
            assert c in comment, (name, c)


@pytest.mark.parametrize("pair", [(48, 0), (0, 0), (224, 0), (256, 0), (16, 0), (64, 64), (64, 128), (32, 32), (96, 32), (-32, 0)])
def test_the_z_entry_points_refuse_other_counts_with_the_rule_in_the_message(pair):
    for call in (_z_fwd, _z_fwd_u8):
        for rays in (8, 0):         # ... before the empty-launch shortcut: a bad count is an error whatever the ray count
            assert call(_frame(*pair, rays=rays)) == -1
            msg = L.dfn_last_error()
            assert b"n_fine == 0" in msg and b"multiple of 32" in msg and b"32 ... 192" in msg, msg
    assert _z_fwd(_frame(*pair), _lib.TIER_F16 | _lib.WIDTH_128) == -1 and b"multiple of 32" in L.dfn_last_error()


def test_the_z_entry_points_refuse_before_any_device_work():
    fr = _frame(96)
    for call in (_z_fwd, _z_fwd_u8):
        assert call(fr, zvals=None) == -1 and b"zvals is NULL" in L.dfn_last_error()
        assert call(fr, _lib.TIER_BF16) == -1 and b"bf16" in L.dfn_last_error()
        assert call(fr, _lib.TIER_BF16 | _lib.WIDTH_128) == -1 and b"bf16" in L.dfn_last_error()
        assert call(fr, bg=None) == -1 and b"no background" in L.dfn_last_error()
        assert L.dfn_last_error().startswith(b"dfn_render_z_fwd:")            # the shared checks report under the entry point's name
    fr2 = _frame(96, fields=2)
    assert _z_fwd(fr2) == -1 and b"fields == 2" in L.dfn_last_error() and L.dfn_last_error().startswith(b"dfn_render_z_fwd:")
    assert _z_fwd(fr2, torso=ONE, bias_t=ONE) == -1 and b"fields == 2" in L.dfn_last_error()          # (rgb_com missing)
    assert _z_fwd_u8(fr2) == -1 and b"fields == 2" in L.dfn_last_error()


@pytest.mark.parametrize("nc", Z_COUNTS)
def test_an_empty_z_launch_returns_ok_at_every_accepted_count_and_tier(nc):
    for tier in Z_TIERS + tuple(t | _lib.WIDTH_128 for t in Z_TIERS):
        assert _z_fwd(_frame(nc, rays=0), tier) == 0, L.dfn_last_error()
        assert _z_fwd_u8(_frame(nc, rays=0), tier) == 0, L.dfn_last_error()
    # with rays to render the next check is reached: the count itself passed (two fields without torso inputs)
    assert _z_fwd(_frame(nc, fields=2)) == -1 and b"fields == 2" in L.dfn_last_error()


def test_the_plain_entry_point_keeps_its_own_count_rule():
    for nc in (96, 160, 192):
        fr = _frame(nc)
        rc = L.dfn_render_fwd(_lib.TIER_F32, C.byref(fr), ONE, None, ONE, None, ONE, None, None, ONE, None, None, None, None, None)
        assert rc == -1 and b"n_coarse must be 32, 64 or 128" in L.dfn_last_error()
        rc = L.dfn_render_rays_fwd(_lib.TIER_F32, C.byref(fr), ONE, None, ONE, None, ONE, None, ONE, None, ONE, None, None, None, None, None)
        assert rc == -1 and b"n_coarse must be 32, 64 or 128" in L.dfn_last_error()


def test_fine_depths_takes_the_hierarchical_pairs_only():
    for nc, nf in ((32, 32), (32, 64), (64, 32), (64, 64), (64, 128)):
        fr = _frame(nc, nf, rays=0)
        assert L.dfn_fine_depths(C.byref(fr), ONE, ONE, None) == 0, L.dfn_last_error()
    for (nc, nf), text in (((64, 0), b"no fine pass"), ((128, 64), b"n_coarse = 32 or 64"), ((32, 128), b"n_fine = 128 needs"),
                           ((96, 32), b"n_coarse must be"), ((64, 96), b"n_fine must be")):
        fr = _frame(nc, nf)
        assert L.dfn_fine_depths(C.byref(fr), ONE, ONE, None) == -1 and text in L.dfn_last_error(), L.dfn_last_error()
    fr = _frame(64, 64)
    assert L.dfn_fine_depths(C.byref(fr), None, ONE, None) == -1 and L.dfn_fine_depths(C.byref(fr), ONE, None, None) == -1


# ---- the command line is untouched -----------------------------------------------------------------------------------------------------
def test_the_cli_flag_tables_are_unchanged():
    p = run_nerf.config_parser()
    assert [n for n, _, _ in run_nerf._EXTRA_FLAGS] == ["hip_tier", "hierarchical", "image_ext", "hip_train_act", "hip_f16_model_psnr"]
    assert run_nerf._OUTPUT_FLAGS == ("save_alpha", "save_depth")
    assert {a.dest for a in p.side._actions} == {"save_alpha", "save_depth"}


# ---- engine.render's argument checks (made before the first device call) -------------------------------------------------------------
def test_engine_render_checks_z_vals_without_a_device():
    pk = types.SimpleNamespace(device=torch.device("cpu"))
    fr = engine.make_frame(8, 8, 10.0, 4.0, 4.0, torch.eye(4).numpy(), None, 0.3, 0.9, ray_count=8, n_coarse=96, n_fine=0, fields=1)
    z = torch.linspace(0.3, 0.9, 96)[None].repeat(8, 1)
    bg = torch.zeros(64, 3)
    for fn, kws in ((engine.render, [{"rays": torch.zeros(8, 6)}, {"want_aux": True}, {"bounds": torch.zeros(8, 2)}]),
                    (engine.render_u8, [{"rays": torch.zeros(8, 6)}, {"want_alpha": True}, {"want_depth": True}])):
        for kw in kws:
            with pytest.raises(ValueError, match="z_vals cannot be combined with " + next(iter(kw))):
                fn(pk, None, fr, bg, z_vals=z, **kw)
        for bad in (z[:, :64], z[:7], z.reshape(-1)):
            with pytest.raises(ValueError, match=r"z_vals must be \[ray_count, n_coarse\] = \[8, 96\]"):
                fn(pk, None, fr, bg, z_vals=bad)
    fr.n_fine = 32
    with pytest.raises(ValueError, match="n_fine == 0"):
        engine.render(pk, None, fr, bg, z_vals=z)
    fr.n_fine, fr.n_coarse = 0, 48
    with pytest.raises(ValueError, match="multiple of 32"):
        engine.render(pk, None, fr, bg, z_vals=z[:, :48])
    fr64 = engine.make_frame(8, 8, 10.0, 4.0, 4.0, torch.eye(4).numpy(), None, 0.3, 0.9, ray_count=8, n_coarse=64, n_fine=0, fields=1)
    with pytest.raises(ValueError, match="no fine pass"):
        engine.render_two_pass(pk, None, pk, None, fr64, bg)
    fr64.n_fine = 64
    with pytest.raises(ValueError, match=r"weights must be \[ray_count, n_coarse\] = \[8, 64\]"):
        engine.fine_depths(fr64, torch.zeros(8, 32))
