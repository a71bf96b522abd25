"""Host-side checks of the ray gradients of the fused training step (dfn_composite_bwd_rays_zg, dfn_composite_bwd_hier_rays_zg,
dfn_points_grad, dfn_rays_grad; training.pinhole_rays, render_train with rays that require grad), no GPU: the C ABI and its ctypes
binding agree, every refusal is found before any device work, pinhole_rays restates get_rays and is differentiable, and the bf16
buffers refuse rays that require grad."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from dfanerf import _lib

NEW = ("dfn_composite_bwd_rays_zg", "dfn_composite_bwd_hier_rays_zg", "dfn_points_grad", "dfn_rays_grad")
one = C.c_void_p(16)                                   # never dereferenced: every call below is refused


def _declared_arg_count(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/dfanerf.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def _frame(n_coarse=64, n_fine=0, fields=2, n=8):
    fr = _lib.DfnFrame()
    fr.ray_count, fr.n_coarse, fr.n_fine, fr.fields, fr.concate_bg = n, n_coarse, n_fine, fields, 1
    return fr


def test_header_declares_and_lib_binds_the_four_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dfanerf.h")).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for name, n_args in zip(NEW, (13, 15, 9, 13)):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        assert _declared_arg_count(hdr, name) == len(getattr(_lib.lib, name).argtypes) == n_args, name
    # the _zg forms are the _rays_z signatures plus d_norm
    for zg, z in zip(NEW[:2], ("dfn_composite_bwd_rays_z", "dfn_composite_bwd_hier_rays_z")):
        assert _declared_arg_count(hdr, zg) == _declared_arg_count(hdr, z) + 1
    doc = hdr[hdr.index("Ray gradients of that step"):hdr.index("int dfn_rays_grad(")]
    for word in ("DEC:277-349", "MAIN:146-179", "DEC:257-275", "MAIN:638-641", "d_norm", "no atomics", "before any device work",
                 "DFN_TIER_F32"):
        assert word in doc, word


def _zg(fr, rays=one, hier=False, zero_buf=None, d_norm=one):
    L = _lib.lib
    if hier:
        rc = L.dfn_composite_bwd_hier_rays_zg(C.byref(fr), rays, None, one, None, one, one, one, one, one, one, zero_buf, 4, d_norm, None)
    else:
        rc = L.dfn_composite_bwd_rays_zg(C.byref(fr), rays, None, one, None, one, one, one, one, zero_buf, 4, d_norm, None)
    return rc, L.dfn_last_error()


def test_zg_entry_points_refuse_before_any_device_work():
    for hier in (False, True):
        name = NEW[hier].encode()
        fr = _frame(64, 128 if hier else 0)
        rc, msg = _zg(fr, d_norm=None, hier=hier)
        assert rc == -1 and name + b": d_norm is NULL" in msg, msg
        rc, msg = _zg(fr, rays=None, hier=hier)
        assert rc == -1 and name + b": rays is NULL" in msg, msg
        rc, msg = _zg(_frame(64, 128 if hier else 0, fields=1), hier=hier)
        assert rc == -1 and name in msg and b"fields == 2" in msg, msg
        rc, msg = _zg(fr, hier=hier, zero_buf=C.c_void_p(20))
        assert rc == -1 and name + b": zero_buf must be 16-byte aligned" in msg, msg
        assert _zg(_frame(64, 128 if hier else 0, n=0), hier=hier)[0] == 0          # an empty launch touches nothing
    for nc, nf in ((48, 0), (64, 64)):
        rc, msg = _zg(_frame(nc, nf))
        assert rc == -1 and b"dfn_composite_bwd_rays_zg: 32, 64 or 128 coarse samples" in msg, msg
    for nc, nf in ((32, 32), (64, 32), (64, 0)):
        rc, msg = _zg(_frame(nc, nf), hier=True)
        assert rc == -1 and b"dfn_composite_bwd_hier_rays_zg: 64 coarse + 64 or 128 fine samples" in msg, msg


def test_points_and_rays_grad_refuse_before_any_device_work():
    L = _lib.lib
    pg = lambda tier=_lib.TIER_F32, field=0, NP=512, a=(one,) * 5: (L.dfn_points_grad(tier, field, NP, *a, None), L.dfn_last_error())
    fr = _frame()
    rg = lambda tier=_lib.TIER_F32, frame=fr, a=(one, None, None, None, one, one, one, one, one, one): \
        (L.dfn_rays_grad(tier, C.byref(frame) if frame is not None else None, *a, None), L.dfn_last_error())
    # the 16-bit tiers: refused with a message that names the f32 tier
    for tier in (_lib.TIER_BF16, _lib.TIER_F16, _lib.TIER_F16X3):
        for call, name in ((pg, b"dfn_points_grad"), (rg, b"dfn_rays_grad")):
            rc, msg = call(tier)
            assert rc == -1 and name in msg and b"ray gradients run in the f32 tier" in msg, msg
    for call, name in ((pg, b"dfn_points_grad"), (rg, b"dfn_rays_grad")):
        rc, msg = call(_lib.TIER_F32 | _lib.WIDTH_128)
        assert rc == -1 and name in msg and b"DFN_WIDTH_128" in msg, msg
    # NULL pointers, one at a time
    for i in range(5):
        rc, msg = pg(a=tuple(None if k == i else one for k in range(5)))
        assert rc == -1 and b"dfn_points_grad: NULL pointer" in msg, (i, msg)
    for i in (0, 4, 5, 6, 7, 8, 9):
        a = [one, None, None, None, one, one, one, one, one, one]
        a[i] = None
        rc, msg = rg(a=tuple(a))
        assert rc == -1 and b"dfn_rays_grad: NULL pointer" in msg, (i, msg)
    rc, msg = rg(frame=None)
    assert rc == -1 and b"dfn_rays_grad: NULL pointer" in msg, msg
    # field, NP, sample counts
    rc, msg = pg(field=3)
    assert rc == -1 and b"dfn_points_grad: bad field" in msg, msg
    for NP in (0, -32, 500):
        rc, msg = pg(NP=NP)
        assert rc == -1 and b"multiple of 32" in msg, msg
    rc, msg = rg(frame=_frame(48, 0))
    assert rc == -1 and b"dfn_rays_grad: 32, 64 or 128 coarse samples" in msg, msg
    rc, msg = rg(frame=_frame(32, 64))
    assert rc == -1 and b"dfn_rays_grad: 64 coarse + 64 or 128 fine samples" in msg, msg
    rc, msg = rg(frame=_frame(64, 128))
    assert rc == -1 and b"z_all and ranks" in msg, msg
    assert rg(frame=_frame(n=0))[0] == 0


def _ulps(a, b):
    """distance in units of the last place of b (float32)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)


def test_pinhole_rays_equal_get_rays_golden_g1(golden):
    from dfanerf import training
    g = golden("g1_rays")
    H, W, focal, cx, cy = g["hwfcxy"]
    idx = torch.from_numpy(g["idx"].astype(np.int64))
    rays = training.pinhole_rays(torch.from_numpy(g["pose_a"]), torch.from_numpy(g["pose_b"]), idx, int(H), int(W), float(focal),
                                 float(cx), float(cy))
    assert rays.shape == (idx.numel(), 12) and rays.dtype == torch.float32 and rays.is_contiguous()
    r = rays.numpy()
    for k, key in enumerate(("rays_o_a", "rays_d_a", "rays_o_b", "rays_d_b")):
        assert float(_ulps(r[:, 3 * k:3 * k + 3], g[key]).max()) <= 1.0, key
    with pytest.raises(ValueError, match="pix is a 1-d integer tensor"):
        training.pinhole_rays(torch.eye(4), torch.eye(4), torch.zeros(3), 4, 4, 1.0, 2.0, 2.0)


def test_pinhole_rays_are_differentiable():
    from dfanerf import training
    torch.manual_seed(0)
    pose = (torch.eye(4)[:3] + 0.1 * torch.randn(3, 4)).double().requires_grad_(True)
    body = (torch.eye(4)[:3] + 0.1 * torch.randn(3, 4)).double().requires_grad_(True)
    pix = torch.tensor([0, 7, 19, 33])
    w = torch.randn(4, 12)
    f = lambda p, b: (training.pinhole_rays(p.float(), b.float(), pix, 6, 7, 9.0, 3.5, 3.0) * w).sum()
    loss = f(pose, body)
    gp, gb = torch.autograd.grad(loss, (pose, body))
    assert float(gp.abs().max()) > 0 and float(gb.abs().max()) > 0
    # the rays are LINEAR in the poses: the gradient is exact and a central difference reproduces it to float32 rounding
    for P, G in ((pose, gp), (body, gb)):
        for (i, j) in ((0, 0), (1, 2), (2, 3), (0, 1)):
            e = torch.zeros_like(P)
            e[i, j] = 0.25
            a = f(pose + e, body) if P is pose else f(pose, body + e)
            b = f(pose - e, body) if P is pose else f(pose, body - e)
            assert abs(float((a - b).detach()) / 0.5 - float(G[i, j])) <= 1e-4 * (1 + abs(float(G[i, j]))), (i, j)
    # the origin block is the pose's translation, the same for every pixel
    r = training.pinhole_rays(pose.float(), body.float(), pix, 6, 7, 9.0, 3.5, 3.0)
    assert torch.equal(r[:, 0:3], pose.float()[:, 3].expand(4, 3)) and torch.equal(r[:, 6:9], body.float()[:, 3].expand(4, 3))


def test_bf16_buffers_refuse_rays_that_require_grad():
    """before any launch: the buffers live on the CPU here, so a call that got past the check could not run at all"""
    from dfanerf import training
    n = 8
    buf = training.TrainBuffers("bf16", n, torch.device("cpu"))
    fr = _frame(64, 0, n=n)
    rays, bg = torch.zeros(n, 12, requires_grad=True), torch.zeros(n, 3)
    sig = (torch.zeros(1, 96), torch.zeros(42), torch.zeros(2, 256), torch.zeros(2, 256))
    with pytest.raises(ValueError, match="ray gradients run in the f32 tier"):
        training.render_train(None, buf, fr, bg, None, *sig, rays=rays)
    # the same rays, detached, pass this check (and every other one: the call then reaches the launches, which a CPU buffer cannot take)
    assert "no rays form" in training.render_train_loss.__doc__
    # Decoder.forward keeps explicit points constants outside the f32 tier (no new refusal for existing callers)
    assert "stay constants" in training.decoder_train.__doc__
