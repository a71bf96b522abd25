"""Host-side checks of the render variant list (csrc/dfn_render_variants.h), no GPU: the one list is well formed, the build's view of
it (render_variants.sh: variant_units, variant_stub) is that same list, and every pairing of a public render / train entry point with a
tier that has NO variant in the list is refused by the entry point - return code and message - before any device work."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from dfanerf import _lib

AMD = os.path.join(ROOT, "dfa-nerf_amd")
HEADER = os.path.join(AMD, "csrc", "dfn_render_variants.h")
TIERS = {"TIER_F32": _lib.TIER_F32, "TIER_BF16": _lib.TIER_BF16, "TIER_F16": _lib.TIER_F16, "TIER_F16X3": _lib.TIER_F16X3}
FLAGS = ("TIER_W128", "TIER_AUX", "TIER_RAYS", "TIER_ZVALS", "TIER_E4M3", "TIER_TRAIN")
ONE = C.c_void_p(16)          # a non-null address that is never dereferenced: every call below is refused before it would be
L = _lib.lib


def parse_variants(path=HEADER):
    """[(name, tier name, frozenset of flag names)] in the order of the file; a DFN_VARIANT line that does not parse is an error"""
    out = []
    for line in open(path):
        if not line.startswith("DFN_VARIANT"):
            continue
        m = re.fullmatch(r"DFN_VARIANT\(([a-z0-9_]+), *(TIER_[A-Z0-9]+), *([A-Z0-9_| ]+)\)\n", line)      # render_variants.sh's own pattern
        assert m, line
        flags = frozenset(f.strip() for f in m.group(3).split("|")) - {"0"}
        assert m.group(2) in TIERS and flags <= set(FLAGS), line
        out.append((m.group(1), m.group(2), flags))
    return out


VARIANTS = parse_variants()
KEYS = {(t, f) for _, t, f in VARIANTS}


def _sh(script):
    return subprocess.run(["bash", "-c", ". ./render_variants.sh; " + script], cwd=AMD, capture_output=True, text=True)


def test_the_list_has_29_unique_names_and_keys():
    assert len(VARIANTS) == 29
    assert len({n for n, _, _ in VARIANTS}) == 29
    assert len(KEYS) == 29


def test_the_build_reads_the_same_list():
    r = _sh("variant_units")
    assert r.returncode == 0 and r.stdout.split("\n") == ["dfn_render_" + n for n, _, _ in VARIANTS] + [""], r
    r = _sh("variant_units TIER_BF16")
    assert r.stdout.split() == ["dfn_render_bf16", "dfn_render_bf16e", "dfn_render_bf16_rays_train", "dfn_render_bf16e_rays_train"]
    # (sourced from another directory: the header is found next to the script, not under the caller's working directory)
    r = subprocess.run(["bash", "-c", ". '%s/render_variants.sh'; variant_units | wc -l" % AMD], cwd="/", capture_output=True, text=True)
    assert r.stdout.strip() == "29", r


def test_variant_stub_writes_three_lines_and_refuses_an_unknown_unit(tmp_path):
    r = _sh("variant_stub dfn_render_f16x3_w128_rays '%s'" % tmp_path)
    assert r.returncode == 0, r
    assert (tmp_path / "dfn_render_f16x3_w128_rays.hip").read_text() == (
        "#define DFN_VARIANT_TIER TIER_F16X3\n#define DFN_VARIANT_FLAGS (TIER_W128|TIER_RAYS)\n#include \"dfn_render_variant.hip\"\n")
    for unit in ("dfn_render_f16x3_w128_ray", "dfn_render_bf16_aux", "dfn_render", "dfn_api", "f32"):
        assert _sh("variant_stub %s '%s'" % (unit, tmp_path)).returncode == 1, unit
    assert sorted(p.name for p in tmp_path.iterdir()) == ["dfn_render_f16x3_w128_rays.hip"]


# ---- entry point x tier pairings without a variant: the entry point's own refusal -------------------------------------------------
def _frame(fields=1, n_fine=0):
    fr = _lib.DfnFrame()
    fr.ray_count, fr.n_coarse, fr.n_fine, fr.fields, fr.concate_bg, fr.H, fr.W = 8, 64, n_fine, fields, 1, 4, 4
    return fr


NET = (ONE, ONE, ONE, ONE)                      # packed_head, packed_torso, bias_head, bias_torso
BGS = (ONE, None)
REC = (ONE, ONE, ONE, ONE, ONE, ONE, ONE)       # rgb_head, rgb_com, samples, act_head, masks_head, act_torso, masks_torso
# inference entry points: name -> (flag of its form, the arguments behind (tier, frame), the name its shared checks report under)
RENDER = {
    "dfn_render_fwd": (None, (*NET, *BGS, None, ONE, ONE, None, None, None, None), "dfn_render_fwd"),
    "dfn_render_fwd_u8": (None, (*NET, *BGS, None, ONE, ONE, None), "dfn_render_fwd"),
    "dfn_render_fwd_aux": ("TIER_AUX", (*NET, *BGS, None, ONE, ONE, ONE, ONE, None), "dfn_render_fwd"),
    "dfn_render_fwd_u8_aux": ("TIER_AUX", (*NET, *BGS, None, ONE, ONE, ONE, ONE, ONE, ONE, None), "dfn_render_fwd"),
    "dfn_render_rays_fwd": ("TIER_RAYS", (*NET, ONE, None, *BGS, ONE, ONE, None, None, None, None), "dfn_render_fwd"),
    "dfn_render_rays_fwd_u8": ("TIER_RAYS", (*NET, ONE, None, *BGS, ONE, ONE, None), "dfn_render_fwd"),
    "dfn_render_z_fwd": ("TIER_ZVALS", (*NET, *BGS, None, ONE, ONE, None, None, None, ONE, None), "dfn_render_z_fwd"),
    "dfn_render_z_fwd_u8": ("TIER_ZVALS", (*NET, *BGS, None, ONE, ONE, ONE, None), "dfn_render_z_fwd"),
}
ONLY = " exist in DFN_TIER_F32 / DFN_TIER_F16 / DFN_TIER_F16X3 only (bf16 is the training tier)"
NO_FORM = {"TIER_AUX": b"dfn_render_fwd_aux: opacity / depth outputs" + ONLY.encode(),
           "TIER_RAYS": b"dfn_render_rays_fwd: caller-supplied rays" + ONLY.encode(),
           "TIER_ZVALS": b"dfn_render_z_fwd: caller-supplied depths" + ONLY.encode()}
NO_W128 = b": DFN_WIDTH_128 applies to DFN_TIER_F32 / DFN_TIER_F16 / DFN_TIER_F16X3 (bf16 is the training tier and stays padded)"
# training entry points: name -> (hierarchical, on rays, the arguments behind (tier, frame), the name its checks report under)
TRAIN = {
    "dfn_train_fwd": (False, False, (*NET, *BGS, ONE, *REC, None), "dfn_train_fwd"),
    "dfn_train_fwd_hier": (True, False, (*NET, *BGS, ONE, *REC, ONE, ONE, None), "dfn_train_fwd_hier"),
    "dfn_train_fwd_loss": (False, False, (*NET, *BGS, ONE, *REC, None, None), "dfn_train_fwd"),
    "dfn_train_fwd_hier_loss": (True, False, (*NET, *BGS, ONE, *REC, ONE, ONE, None, None), "dfn_train_fwd_hier"),
    "dfn_train_rays_fwd": (False, True, (*NET, ONE, None, *BGS, *REC, None), "dfn_train_rays_fwd"),
    "dfn_train_rays_fwd_hier": (True, True, (*NET, ONE, None, *BGS, *REC, ONE, ONE, None), "dfn_train_rays_fwd_hier"),
}
TRAIN_NO_W128 = (b": DFN_WIDTH_128 selects the 128-wide INFERENCE program (dfn_packed_bytes, dfn_pack_weights, dfn_pack_plan, "
                 b"dfn_bias_floats, dfn_fold_bias, dfn_render_fwd, dfn_render_fwd_u8, dfn_decoder_fwd); training and everything else "
                 b"stay on the padded 256-wide layout")
INFERENCE_ONLY = b": DFN_TIER_F16 / DFN_TIER_F16X3 are inference only; the training step runs in DFN_TIER_F32 / DFN_TIER_BF16"


def _refused(name, tier, fr, args, message):
    assert getattr(L, name)(tier, C.byref(fr), *args) == -1, (name, tier)
    assert L.dfn_last_error() == message, (name, tier, L.dfn_last_error())


@pytest.mark.parametrize("name", sorted(RENDER))
def test_a_render_entry_point_refuses_the_tiers_without_its_variant(name):
    form, args, who = RENDER[name]
    missing = 0
    for tname, tier in TIERS.items():
        flags = frozenset([form] if form else [])
        if form and (tname, flags) not in KEYS:         # the form does not exist in this tier at all
            _refused(name, tier, _frame(), args, NO_FORM[form])
            missing += 1
        if (tname, flags | {"TIER_W128"}) not in KEYS:   # ... or not in its 128-wide program
            _refused(name, tier | _lib.WIDTH_128, _frame(), args, who.encode() + NO_W128)
            missing += 1
    # today's list: bf16 is the one tier without the inference forms and without a 128-wide program
    assert missing == (2 if form else 1), name


@pytest.mark.parametrize("name", sorted(TRAIN))
def test_a_train_entry_point_refuses_the_tiers_without_its_variant(name):
    hier, on_rays, args, who = TRAIN[name]
    fr = _frame(fields=2, n_fine=64 if hier else 0)
    flags = frozenset(["TIER_RAYS", "TIER_TRAIN"] if on_rays else [])
    for tname, tier in TIERS.items():
        # no training kernel is 128-wide (the TIER_W128 units are inference only): DFN_WIDTH_128 is refused in every tier
        assert not on_rays or (tname, flags | {"TIER_W128"}) not in KEYS
        _refused(name, tier | _lib.WIDTH_128, fr, args, who.encode() + TRAIN_NO_W128)
        if on_rays and (tname, flags) not in KEYS:
            assert tname in ("TIER_F16", "TIER_F16X3")
            _refused(name, tier, fr, args, who.encode() + INFERENCE_ONLY)
    if on_rays:
        assert ("TIER_F32", flags) in KEYS and ("TIER_BF16", flags) in KEYS and ("TIER_BF16", flags | {"TIER_E4M3"}) in KEYS
