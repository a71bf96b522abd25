"""Host-side checks of the caller-supplied-rays entry points (dfn_render_rays_fwd, dfn_render_rays_fwd_u8; no GPU): the C ABI and
its ctypes binding agree, the argument errors are found before any device work, and engine.pack_rays lays the rows out as the
header documents them (o_head, d_head[, o_torso, d_torso])."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from dfanerf import _lib

RAYS_SYMBOLS = ("dfn_render_rays_fwd", "dfn_render_rays_fwd_u8")


def _declared_arg_count(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/dfanerf.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_declares_and_lib_binds_the_rays_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dfanerf.h")).read()
    # dfn_render_fwd's arguments with (rays, bounds) in place of pix_index: one more each
    for name, n_args, plain in zip(RAYS_SYMBOLS, (16, 13), ("dfn_render_fwd", "dfn_render_fwd_u8")):
        assert name in _lib.EXPORTS
        fn = getattr(_lib.lib, name)
        assert _declared_arg_count(hdr, name) == len(fn.argtypes) == n_args == _declared_arg_count(hdr, plain) + 1, name
    # the header says which frame fields a rays launch ignores, and that there is no aux / training form
    doc = hdr[hdr.index("CALLER-SUPPLIED rays"):hdr.index("int dfn_render_rays_fwd(")]
    for word in ("IGNORED", "pose_body", "ray_begin", "HELP:449-465", "MAIN:612-619", "NO aux form", "NO training form"):
        assert word in doc, word


def test_rays_entry_points_refuse_before_any_device_work():
    """argument errors are found before the first HIP call, so they can be checked without a GPU"""
    fr = _lib.DfnFrame()
    fr.ray_count, fr.n_coarse, fr.n_fine, fr.fields, fr.concate_bg = 8, 64, 0, 1, 1        # (H = W = 0: ignored by a rays launch)
    one = C.c_void_p(16)                                   # never dereferenced: every call below is refused
    L = _lib.lib
    head = (C.byref(fr), one, None, one, None)
    f32_out = (one, None, None, None, None, None)
    u8_out = (one, None, None)
    # NULL rays
    assert L.dfn_render_rays_fwd(_lib.TIER_F32, *head, None, None, one, None, *f32_out) == -1 and b"rays is NULL" in L.dfn_last_error()
    assert L.dfn_render_rays_fwd_u8(_lib.TIER_F16, *head, None, one, one, None, *u8_out) == -1 and b"rays is NULL" in L.dfn_last_error()
    # bf16 is the training tier
    assert L.dfn_render_rays_fwd(_lib.TIER_BF16, *head, one, None, one, None, *f32_out) == -1 and b"bf16" in L.dfn_last_error()
    assert L.dfn_render_rays_fwd_u8(_lib.TIER_BF16, *head, one, None, one, None, *u8_out) == -1 and b"bf16" in L.dfn_last_error()
    assert L.dfn_render_rays_fwd(_lib.TIER_BF16 | _lib.WIDTH_128, *head, one, None, one, None, *f32_out) == -1
    # dfn_render_fwd's own checks still apply: sample counts, the hierarchical mode's n_coarse, the background, fields
    fr.n_coarse, fr.n_fine = 32, 128
    assert L.dfn_render_rays_fwd(_lib.TIER_F32, *head, one, one, one, None, *f32_out) == -1 and b"n_coarse = 64" in L.dfn_last_error()
    fr.n_coarse, fr.n_fine = 48, 0
    assert L.dfn_render_rays_fwd(_lib.TIER_F16X3 | _lib.WIDTH_128, *head, one, None, one, None, *f32_out) == -1
    fr.n_coarse = 64
    assert L.dfn_render_rays_fwd(_lib.TIER_F32, *head, one, None, None, None, *f32_out) == -1 and b"background" in L.dfn_last_error()
    fr.fields = 2                                          # torso inputs / rgb_com missing
    assert L.dfn_render_rays_fwd(_lib.TIER_F32, *head, one, None, one, None, *f32_out) == -1 and b"fields == 2" in L.dfn_last_error()
    # an empty launch is not an error, and touches nothing
    fr.fields, fr.ray_count = 1, 0
    assert L.dfn_render_rays_fwd(_lib.TIER_F32, *head, one, None, one, None, *f32_out) == 0


def test_pack_rays_layout():
    from dfanerf import engine
    rng = np.random.RandomState(0)
    o_h, d_h, o_t, d_t = [torch.from_numpy(rng.randn(7, 3).astype(np.float32)) for _ in range(4)]
    one = engine.pack_rays(o_h, d_h)
    assert one.shape == (7, 6) and one.dtype == torch.float32 and one.is_contiguous()
    assert torch.equal(one[:, :3], o_h) and torch.equal(one[:, 3:], d_h)
    two = engine.pack_rays(o_h, d_h, o_t, d_t)
    assert two.shape == (7, 12) and two.dtype == torch.float32 and two.is_contiguous()
    assert torch.equal(two, torch.cat([o_h, d_h, o_t, d_t], 1))
    # image-shaped tensors as get_rays returns them, other dtypes, strided views
    img = engine.pack_rays(o_h.double().reshape(7, 1, 3), d_h.reshape(1, 7, 3))
    assert torch.equal(img, one)
    wide = torch.from_numpy(rng.randn(7, 6).astype(np.float32))
    sl = engine.pack_rays(wide[:, :3], wide[:, 3:], wide[:, 3:], wide[:, :3])
    assert sl.is_contiguous() and torch.equal(sl[:, :6], wide) and torch.equal(sl[:, 6:9], wide[:, 3:])
    assert engine.pack_rays(o_h.numpy(), d_h.numpy()).shape == (7, 6)


def test_pack_rays_refuses_mismatched_input():
    from dfanerf import engine
    a, b = torch.zeros(7, 3), torch.zeros(6, 3)
    with pytest.raises(ValueError, match="mismatched"):
        engine.pack_rays(a, b)
    with pytest.raises(ValueError, match="mismatched"):
        engine.pack_rays(a, a, a, b)
    with pytest.raises(ValueError, match="pair"):
        engine.pack_rays(a, a, o_torso=a)
    with pytest.raises(ValueError, match="pair"):
        engine.pack_rays(a, a, d_torso=a)
    with pytest.raises(ValueError, match=r"\[\.\.\., 3\]"):
        engine.pack_rays(torch.zeros(7, 4), torch.zeros(7, 4))
