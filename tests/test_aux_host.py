"""Host-side checks of the opacity / expected-depth outputs (dfn_render_fwd_aux, dfn_render_fwd_u8_aux; no GPU): the C ABI and its
ctypes binding agree, the drop-in CLI takes --save_alpha / --save_depth without disturbing the reference's flags, and the
documented summation order (include/dfanerf.h; csrc/dfn_render_kernels.h, TIER_AUX), restated in numpy, meets the error bound the
GPU test holds the kernels to."""
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from dfanerf import _lib, run_nerf

AUX_SYMBOLS = ("dfn_render_fwd_aux", "dfn_render_fwd_u8_aux")


def _declared_arg_count(hdr, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/dfanerf.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_declares_and_lib_binds_the_aux_entry_points():
    hdr = open(os.path.join(ROOT, "include", "dfanerf.h")).read()
    for name, n_args in zip(AUX_SYMBOLS, (14, 16)):
        assert name in _lib.EXPORTS
        fn = getattr(_lib.lib, name)
        assert _declared_arg_count(hdr, name) == len(fn.argtypes) == n_args, name
    # the aux forms extend the plain ones: dfn_render_fwd's inputs, two aux arrays instead of the three per-sample ones; the u8
    # form grows by the four per-ray planes
    assert _declared_arg_count(hdr, "dfn_render_fwd") == 15 and _declared_arg_count(hdr, "dfn_render_fwd_u8") == 12
    assert b"0.4" in _lib.lib.dfn_version() and "0.4:" in hdr


def test_aux_entry_points_refuse_before_any_device_work():
    """argument errors are found before the first HIP call, so they can be checked without a GPU"""
    fr = _lib.DfnFrame()
    fr.H, fr.W, fr.ray_count, fr.n_coarse, fr.n_fine, fr.fields, fr.concate_bg = 8, 8, 8, 64, 0, 1, 1
    import ctypes as C
    one = C.c_void_p(16)                                   # never dereferenced: every call below is refused
    L = _lib.lib
    args = (C.byref(fr), one, None, one, None, one, None, None, one, None)
    assert L.dfn_render_fwd_aux(_lib.TIER_F32, *args, None, None, None) == -1 and b"aux_head" in L.dfn_last_error()
    assert L.dfn_render_fwd_aux(_lib.TIER_BF16, *args, one, None, None) == -1 and b"bf16" in L.dfn_last_error()
    assert L.dfn_render_fwd_aux(_lib.TIER_BF16 | _lib.WIDTH_128, *args, one, None, None) == -1
    assert L.dfn_render_fwd_u8_aux(_lib.TIER_F16, *args, None, None, None, None, None) == -1 and b"neither" in L.dfn_last_error()
    assert L.dfn_render_fwd_u8_aux(_lib.TIER_BF16, *args, one, None, one, None, None) == -1 and b"bf16" in L.dfn_last_error()
    fr.fields = 2
    args2 = (C.byref(fr), one, one, one, one, one, None, None, one, one)
    assert L.dfn_render_fwd_aux(_lib.TIER_F16, *args2, one, None, None) == -1 and b"aux_com" in L.dfn_last_error()
    assert L.dfn_render_fwd_u8_aux(_lib.TIER_F16, *args2, one, None, None, None, None) == -1 and b"alpha8_com" in L.dfn_last_error()
    assert L.dfn_render_fwd_u8_aux(_lib.TIER_F16, *args2, None, None, one, None, None) == -1
    assert L.dfn_render_fwd_u8_aux(_lib.TIER_F16, *args2, None, one, one, one, None) == -1 and b"_head pointer" in L.dfn_last_error()


def test_cli_takes_the_flags_and_leaves_the_reference_flags_alone():
    want = json.load(open(os.path.join(GOLDEN, "g11_cli_flags.json")))
    assert len(want) == 89
    base = "--expname t --concate_bg --dim_signal=96 --n_object=1 --render_person --hip_tier f16".split()
    a0 = run_nerf.config_parser().parse_args(base)
    assert a0.save_alpha is False and a0.save_depth is False
    for extra in (["--save_alpha"], ["--save_depth"], ["--save_alpha", "--save_depth"]):
        a = run_nerf.config_parser().parse_args(base[:3] + extra + base[3:])
        assert a.save_alpha is ("--save_alpha" in extra) and a.save_depth is ("--save_depth" in extra)
        for f in want:                                       # every one of the reference's 89 flags parses as without the switches
            assert getattr(a, f["name"]) == getattr(a0, f["name"]), f
        assert {k: v for k, v in vars(a).items() if not k.startswith("save_")} == \
            {k: v for k, v in vars(a0).items() if not k.startswith("save_")}
        run_nerf.check_supported(a)
    text = run_nerf.config_parser().format_help()
    assert "--save_alpha" in text and "--save_depth" in text and "I;16" in text
    with pytest.raises(SystemExit, match="bf16"):
        run_nerf.check_supported(run_nerf.config_parser().parse_args(base[:-1] + ["bf16", "--save_depth"]))


def aux_sums_twin(w, z, concate_bg=True):
    """include/dfanerf.h (dfn_render_fwd_aux), as csrc/dfn_render_kernels.h computes it, in numpy f32: per 32-sample tile each lane
    forms w and the rounded product w * z (0 outside FG), the lanes combine by a butterfly at XOR distances 16, 8, 4, 2, 1, the
    tiles add into the running sums in tile order.  w, z [rays, S] f32 -> acc, depth [rays] f32."""
    w, z = np.asarray(w, np.float32), np.asarray(z, np.float32)
    R, S = w.shape
    assert S % 32 == 0
    fg = np.ones(S, bool)
    if concate_bg:
        fg[S - 1] = False
    lanes = np.arange(32)
    acc, dep = np.zeros(R, np.float32), np.zeros(R, np.float32)
    for t in range(S // 32):
        sl = slice(32 * t, 32 * t + 32)
        a = np.where(fg[sl], w[:, sl], np.float32(0))
        d = np.where(fg[sl], w[:, sl] * z[:, sl], np.float32(0))
        for dlt in (16, 8, 4, 2, 1):
            a = a + a[:, lanes ^ dlt]
            d = d + d[:, lanes ^ dlt]
        assert (a == a[:, :1]).all() and (d == d[:, :1]).all()      # every lane ends with the same value
        acc, dep = acc + a[:, 0], dep + d[:, 0]
    assert acc.dtype == np.float32 and dep.dtype == np.float32
    return acc, dep


@pytest.mark.parametrize("S", [32, 64, 128, 192])
@pytest.mark.parametrize("concate_bg", [True, False])
def test_documented_sum_order_meets_the_bound(S, concate_bg):
    """random compositing weights (non-negative, summing to <= 1) and sorted depths in [z_near, z_far]: the tile-order f32 sums against
    float64 within S * 2^-23 (acc) and z_far * S * 2^-23 (depth) - at most S roundings of partial sums <= 1, each <= 2^-24, doubled"""
    rng = np.random.RandomState(S + int(concate_bg))
    z_near, z_far = np.float32(0.3), np.float32(0.9)
    alpha = rng.rand(512, S).astype(np.float32) ** 6
    alpha[::7] = 0                                           # empty rays: everything lands on the last sample
    alpha[:, -1] = 1
    trans = np.cumprod(np.concatenate([np.ones((512, 1), np.float32), 1 - alpha[:, :-1]], 1), 1, dtype=np.float32)
    w = (alpha * trans).astype(np.float32)
    z = np.sort(rng.uniform(z_near, z_far, (512, S)).astype(np.float32), 1)
    acc, dep = aux_sums_twin(w, z, concate_bg)
    n_fg = S - 1 if concate_bg else S
    acc64 = w[:, :n_fg].astype(np.float64).sum(1)
    dep64 = (w[:, :n_fg].astype(np.float64) * z[:, :n_fg]).sum(1)
    assert np.abs(acc - acc64).max() <= S * 2.0 ** -23
    assert np.abs(dep - dep64).max() <= float(z_far) * S * 2.0 ** -23
    assert acc64.max() > 0.9 and (dep64 <= acc64 * float(z_far) + 1e-12).all()
    if concate_bg:
        assert acc64.min() < 0.1                              # the empty rays: all of the weight is the background plane's
    if not concate_bg:
        assert np.abs(acc - 1.0).max() <= 1e-5
