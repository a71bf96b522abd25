"""Host-side checks of the hierarchical mode's sample counts (no GPU): the pairs (n_coarse, n_fine) the forward entry points take
are 32+32, 32+64, 64+32, 64+64 and 64+128 (include/dfanerf.h, DfnFrame); the command line takes the three new ones for a render
(--render_person) and refuses them for a training run, whose backward is 64 + 64 | 128.  The ABI's argument checks run before any
HIP call, so they can be made here."""
import ctypes as C

import pytest

from dfanerf import _lib, run_nerf

NEW_PAIRS = [(32, 32), (32, 64), (64, 32)]
OLD_PAIRS = [(64, 64), (64, 128)]
BASE = "--expname t --z_dim 256 --dim_signal 96 --n_object 1 --use_deformation_field --n_feat 256 "


def _parse(extra):
    return run_nerf.config_parser().parse_args((BASE + extra).split())


@pytest.mark.parametrize("nc,nf", NEW_PAIRS + OLD_PAIRS)
def test_check_supported_accepts_every_pair_for_a_render(nc, nf):
    run_nerf.check_supported(_parse(f"--render_person --hierarchical --N_samples {nc} --N_importance {nf}"))
    for tier in ("f16", "f16x3", "f32", "auto"):
        run_nerf.check_supported(_parse(f"--render_person --hierarchical --N_samples {nc} --N_importance {nf} --hip_tier {tier}"))


@pytest.mark.parametrize("nc,nf", NEW_PAIRS)
def test_check_supported_refuses_the_new_pairs_for_a_training_run_and_says_why(nc, nf):
    with pytest.raises(SystemExit, match="unsupported configuration") as e:
        run_nerf.check_supported(_parse(f"--hierarchical --N_samples {nc} --N_importance {nf}"))
    msg = str(e.value)
    assert "the hierarchical training step is 64 + 64 | 128" in msg and "--render_person" in msg
    assert f"--N_samples {nc} --N_importance {nf}" in msg


def test_check_supported_keeps_the_training_pairs_and_the_coarse_only_counts():
    for nc, nf in OLD_PAIRS:
        run_nerf.check_supported(_parse(f"--hierarchical --N_samples {nc} --N_importance {nf}"))
    for nc in (32, 64, 128):                     # without --hierarchical N_importance (default 128) is not used
        run_nerf.check_supported(_parse(f"--N_samples {nc}"))
        run_nerf.check_supported(_parse(f"--render_person --N_samples {nc}"))


@pytest.mark.parametrize("extra", ["--hierarchical --N_importance 96", "--hierarchical --N_samples 128",
                                   "--hierarchical --N_samples 32 --N_importance 128", "--hierarchical --N_samples 128 --N_importance 64",
                                   "--hierarchical --N_samples 64 --N_importance 16", "--hierarchical --N_samples 48 --N_importance 32"])
def test_check_supported_refuses_the_other_counts_for_a_render_too(extra):
    with pytest.raises(SystemExit, match="unsupported configuration"):
        run_nerf.check_supported(_parse("--render_person " + extra))
    with pytest.raises(SystemExit, match="unsupported configuration"):
        run_nerf.check_supported(_parse(extra))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
ONE = C.c_void_p(16)          # a non-null address that is never dereferenced: every call below returns before it would be


def _frame(nc, nf, fields=1, rays=8):
    fr = _lib.DfnFrame()
    fr.ray_count, fr.n_coarse, fr.n_fine, fr.fields, fr.concate_bg, fr.H, fr.W = rays, nc, nf, fields, 1, 4, 4
    return fr


def _render_fwd(fr, tier=_lib.TIER_F32):
    # (one field: weights, bias, a float background, rgb_head)
    return _lib.lib.dfn_render_fwd(tier, C.byref(fr), ONE, None, ONE, None, ONE, None, None, ONE, None, None, None, None, None)


def _train_fwd_hier(fr, tier=_lib.TIER_F32):
    return _lib.lib.dfn_train_fwd_hier(tier, C.byref(fr), ONE, ONE, ONE, ONE, ONE, None, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE,
                                       None)


REFUSED = [((32, 128), b"n_fine = 128 needs n_coarse = 64"), ((64, 96), b"n_fine must be 0, 32, 64 or 128"),
           ((128, 64), b"needs n_coarse = 32 or 64"), ((128, 128), b"n_fine = 128 needs n_coarse = 64"), ((96, 64), b"n_coarse must be 32, 64 or 128"),
           ((48, 0), b"n_coarse must be 32, 64 or 128"), ((32, 16), b"n_fine must be"), ((64, 192), b"n_fine must be")]


@pytest.mark.parametrize("pair,text", REFUSED)
def test_the_abi_refuses_the_other_pairs_with_the_rule_in_the_message(pair, text):
    L = _lib.lib
    assert _render_fwd(_frame(*pair)) == -1 and text in L.dfn_last_error(), L.dfn_last_error()
    assert _render_fwd(_frame(*pair), _lib.TIER_F16 | _lib.WIDTH_128) == -1 and text in L.dfn_last_error()
    # ... before the empty-launch shortcut: a bad pair is an error whatever the ray count
    assert _render_fwd(_frame(*pair, rays=0)) == -1
    # the u8 / aux / rays forms go through the same check
    fr = _frame(*pair)
    assert L.dfn_render_fwd_u8(_lib.TIER_F16, C.byref(fr), ONE, None, ONE, None, ONE, None, None, ONE, None, None) == -1
    assert text in L.dfn_last_error()
    assert L.dfn_render_fwd_aux(_lib.TIER_F16X3, C.byref(fr), ONE, None, ONE, None, ONE, None, None, ONE, None, ONE, None, None) == -1
    assert text in L.dfn_last_error()
    assert L.dfn_render_rays_fwd(_lib.TIER_F32, C.byref(fr), ONE, None, ONE, None, ONE, None, ONE, None, ONE, None, None, None, None,
                                 None) == -1
    assert text in L.dfn_last_error()
    if pair[1] > 0:            # the recording forward takes the renderer's pairs, and refuses what it refuses
        assert _train_fwd_hier(_frame(*pair, fields=2)) == -1 and text in L.dfn_last_error(), L.dfn_last_error()


@pytest.mark.parametrize("nc,nf", NEW_PAIRS + OLD_PAIRS)
def test_an_empty_launch_at_every_accepted_pair_returns_ok(nc, nf):
    for tier in (_lib.TIER_F32, _lib.TIER_F16, _lib.TIER_F16X3, _lib.TIER_BF16, _lib.TIER_F16 | _lib.WIDTH_128):
        assert _render_fwd(_frame(nc, nf, rays=0), tier) == 0, _lib.lib.dfn_last_error()
    for tier in (_lib.TIER_F32, _lib.TIER_BF16):
        assert _train_fwd_hier(_frame(nc, nf, fields=2, rays=0), tier) == 0, _lib.lib.dfn_last_error()
    # with rays to render the next check is reached: the pair itself passed (two fields without torso inputs)
    assert _render_fwd(_frame(nc, nf, fields=2)) == -1 and b"fields == 2" in _lib.lib.dfn_last_error()


def test_the_recording_forward_still_needs_a_fine_pass_and_two_fields():
    L = _lib.lib
    assert _train_fwd_hier(_frame(64, 0, fields=2)) == -1 and b"n_fine > 0" in L.dfn_last_error()
    assert _train_fwd_hier(_frame(32, 64, fields=1)) == -1 and b"two fields" in L.dfn_last_error()


@pytest.mark.parametrize("nc,nf", NEW_PAIRS)
def test_the_hierarchical_backward_and_the_training_buffers_stay_at_64_coarse(nc, nf):
    """training at the new pairs is not built: the compositing backward refuses them, and so does TrainBuffers - before it
    allocates anything"""
    from dfanerf import training
    L = _lib.lib
    fr = _frame(nc, nf, fields=2)
    assert L.dfn_composite_bwd_hier(C.byref(fr), ONE, ONE, None, ONE, ONE, ONE, ONE, ONE, ONE, None) == -1
    assert b"64 coarse + 64 or 128 fine" in L.dfn_last_error()
    with pytest.raises(ValueError, match="TrainBuffers"):
        training.TrainBuffers("f32", 64, "cpu", n_fine=nf, n_coarse=nc)
