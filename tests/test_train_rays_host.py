"""Host-side checks of the training step on caller-supplied rays (dfn_train_rays_fwd, dfn_train_rays_fwd_hier,
dfn_composite_bwd_rays_z, dfn_composite_bwd_hier_rays_z; training.render_train(rays=, bounds=)), no GPU: the C ABI and its ctypes
binding agree, every refusal is found before any device work, and render_train names the argument it refuses."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from dfanerf import _lib

FWD = ("dfn_train_rays_fwd", "dfn_train_rays_fwd_hier")
BWD = ("dfn_composite_bwd_rays_z", "dfn_composite_bwd_hier_rays_z")


def _declared_arg_count(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/dfanerf.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_declares_and_lib_binds_the_four_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dfanerf.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    # (rays, bounds) in place of pix_index: one argument more than the plain call
    for name, n_args, plain in zip(FWD + BWD, (18, 20, 12, 14),
                                   ("dfn_train_fwd", "dfn_train_fwd_hier", "dfn_composite_bwd_z", "dfn_composite_bwd_hier_z")):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        fn = getattr(_lib.lib, name)
        assert _declared_arg_count(hdr, name) == len(fn.argtypes) == n_args == _declared_arg_count(hdr, plain) + 1, name
    doc = hdr[hdr.index("The training step on CALLER-SUPPLIED rays"):hdr.index("int dfn_train_rays_fwd(")]
    for word in ("o_head[3], d_head[3], o_torso[3], d_torso[3]", "IGNORED", "HELP:449-465", "MAIN:612-619", "NO _loss forms",
                 "fields == 2", "before any device work", "bit for bit"):
        assert word in doc, word
    # the inference comment no longer says that training on rays does not exist
    rays_doc = hdr[hdr.index("CALLER-SUPPLIED rays"):hdr.index("int dfn_render_rays_fwd(")]
    assert "dfn_train_rays_fwd" in rays_doc and "NO training form of these" not in rays_doc


def _frame(n_coarse=64, n_fine=0, fields=2, n=8):
    fr = _lib.DfnFrame()
    fr.ray_count, fr.n_coarse, fr.n_fine, fr.fields, fr.concate_bg = n, n_coarse, n_fine, fields, 1      # (H = W = 0: ignored)
    return fr


one = C.c_void_p(16)                                   # never dereferenced: every call below is refused


def _fwd(tier, fr, rays=one, hier=False):
    L = _lib.lib
    head = (tier, C.byref(fr), one, one, one, one, rays, None, one, None, one, one, one, one, one, one, one)
    rc = L.dfn_train_rays_fwd_hier(*head, one, one, None) if hier else L.dfn_train_rays_fwd(*head, None)
    return rc, L.dfn_last_error()


def _bwd(fr, rays=one, hier=False, zero_buf=None):
    L = _lib.lib
    if hier:
        rc = L.dfn_composite_bwd_hier_rays_z(C.byref(fr), rays, None, one, None, one, one, one, one, one, one, zero_buf, 4, None)
    else:
        rc = L.dfn_composite_bwd_rays_z(C.byref(fr), rays, None, one, None, one, one, one, one, zero_buf, 4, None)
    return rc, L.dfn_last_error()


def test_forward_entry_points_refuse_before_any_device_work():
    for hier in (False, True):
        name = FWD[hier].encode()
        fr = _frame(64, 128 if hier else 0)
        # NULL rays
        rc, msg = _fwd(_lib.TIER_F32, fr, rays=None, hier=hier)
        assert rc == -1 and name + b": rays is NULL" in msg, msg
        # tiers that do not train
        for tier in (_lib.TIER_F16, _lib.TIER_F16X3):
            rc, msg = _fwd(tier, fr, hier=hier)
            assert rc == -1 and name in msg and b"inference only" in msg, msg
        # the 128-wide program is inference only
        for tier in (_lib.TIER_F32, _lib.TIER_BF16):
            rc, msg = _fwd(tier | _lib.WIDTH_128, fr, hier=hier)
            assert rc == -1 and name in msg and b"DFN_WIDTH_128" in msg, msg
        # the e4m3 recorder is the bf16 tier's
        rc, msg = _fwd(_lib.TIER_F32 | _lib.TRAIN_ACT_E4M3, fr, hier=hier)
        assert rc == -1 and name in msg and b"DFN_TRAIN_ACT_E4M3 applies to DFN_TIER_BF16 only" in msg, msg
        # one field
        for tier in (_lib.TIER_F32, _lib.TIER_BF16, _lib.TIER_BF16 | _lib.TRAIN_ACT_E4M3):
            rc, msg = _fwd(tier, _frame(64, 128 if hier else 0, fields=1), hier=hier)
            assert rc == -1 and name in msg and b"fields == 2" in msg, msg
        # an empty launch is not an error, and touches nothing
        assert _fwd(_lib.TIER_BF16, _frame(64, 128 if hier else 0, n=0), hier=hier)[0] == 0
    # counts the plain forms refuse
    for nc, nf in ((48, 0), (64, 128), (64, 64)):
        rc, msg = _fwd(_lib.TIER_F32, _frame(nc, nf))
        assert rc == -1 and b"dfn_train_rays_fwd: 32, 64 or 128 coarse samples" in msg, msg
    rc, msg = _fwd(_lib.TIER_BF16, _frame(64, 0), hier=True)
    assert rc == -1 and b"dfn_train_rays_fwd_hier: n_fine > 0" in msg, msg
    for nc, nf, word in ((32, 128, b"n_coarse = 64"), (64, 96, b"n_fine must be"), (128, 64, b"n_coarse = 32 or 64")):
        rc, msg = _fwd(_lib.TIER_BF16, _frame(nc, nf), hier=True)
        assert rc == -1 and b"dfn_train_rays_fwd_hier" in msg and word in msg, msg
    # the pairs counts_ok allows pass the count checks (and fail later, on the missing background, still before any device work)
    L = _lib.lib
    for nc, nf in ((32, 32), (32, 64), (64, 32), (64, 64), (64, 128)):
        fr = _frame(nc, nf)
        rc = L.dfn_train_rays_fwd_hier(_lib.TIER_F32, C.byref(fr), one, one, one, one, one, None, None, None, one, one, one, one, one,
                                       one, one, one, one, None)
        assert rc == -1 and b"dfn_train_rays_fwd_hier: no background given" in L.dfn_last_error()


def test_backward_entry_points_refuse_before_any_device_work():
    for hier in (False, True):
        name = BWD[hier].encode()
        fr = _frame(64, 128 if hier else 0)
        rc, msg = _bwd(fr, rays=None, hier=hier)
        assert rc == -1 and name + b": rays is NULL" in msg, msg
        rc, msg = _bwd(_frame(64, 128 if hier else 0, fields=1), hier=hier)
        assert rc == -1 and name in msg and b"fields == 2" in msg, msg
        rc, msg = _bwd(fr, hier=hier, zero_buf=C.c_void_p(20))
        assert rc == -1 and name + b": zero_buf must be 16-byte aligned" in msg, msg
        assert _bwd(_frame(64, 128 if hier else 0, n=0), hier=hier)[0] == 0
    for nc, nf in ((48, 0), (64, 64)):
        rc, msg = _bwd(_frame(nc, nf))
        assert rc == -1 and b"dfn_composite_bwd_rays_z: 32, 64 or 128 coarse samples" in msg, msg
    # the hierarchical backward is 64 + 64 | 128, as dfn_composite_bwd_hier is
    for nc, nf in ((32, 32), (32, 64), (64, 32), (64, 0)):
        rc, msg = _bwd(_frame(nc, nf), hier=True)
        assert rc == -1 and b"dfn_composite_bwd_hier_rays_z: 64 coarse + 64 or 128 fine samples" in msg, msg


def test_existing_entry_points_keep_their_refusals():
    """dfn_render_rays_fwd still refuses bf16, dfn_composite_bwd_hier still refuses the other pairs"""
    L = _lib.lib
    fr = _frame(64, 0, fields=1)
    assert L.dfn_render_rays_fwd(_lib.TIER_BF16, C.byref(fr), one, None, one, None, one, None, one, None, one, None, None, None, None,
                                 None) == -1 and b"bf16" in L.dfn_last_error()
    fr = _frame(32, 32)
    assert L.dfn_composite_bwd_hier(C.byref(fr), None, one, None, one, one, one, one, one, one, None) == -1
    assert b"dfn_composite_bwd_hier: 64 coarse + 64 or 128 fine samples" in L.dfn_last_error()


def test_render_train_refuses_bad_rays_arguments_by_name():
    """before any launch: the buffers live on the CPU here, so a call that got past the checks could not run at all"""
    from dfanerf import training
    n = 8
    buf = training.TrainBuffers("f32", n, torch.device("cpu"))
    fr = _frame(64, 0, n=n)
    rays, bg, pix = torch.zeros(n, 12), torch.zeros(n, 3), torch.zeros(n, dtype=torch.int32)
    sig = (torch.zeros(1, 96), torch.zeros(42), torch.zeros(2, 256), torch.zeros(2, 256))
    call = lambda bg_, pix_, **kw: training.render_train(None, buf, fr, bg_, pix_, *sig, **kw)
    with pytest.raises(ValueError, match="pix_index"):
        call(bg, pix, rays=rays)
    with pytest.raises(ValueError, match=r"rays must be .*\[8, 12\]"):
        call(bg, None, rays=torch.zeros(n, 6))
    with pytest.raises(ValueError, match=r"rays must be"):
        call(bg, None, rays=torch.zeros(n + 1, 12))
    with pytest.raises(ValueError, match=r"rays must be"):
        call(bg, None, rays=torch.zeros(n, 24)[:, ::2])
    with pytest.raises(ValueError, match=r"rays must be"):
        call(bg, None, rays=rays.double())
    with pytest.raises(ValueError, match=r"bg must be .*\[8, 3\]"):
        call(torch.zeros(n + 3, 3), None, rays=rays)
    with pytest.raises(ValueError, match=r"bounds must be .*\[8, 2\]"):
        call(bg, None, rays=rays, bounds=torch.zeros(n, 3))
    with pytest.raises(ValueError, match="rays is None"):
        call(bg, None, bounds=torch.zeros(n, 2))
    assert "no rays form" in training.render_train_loss.__doc__
