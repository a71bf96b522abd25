"""--hip_tier f16x3 through the drop-in driver (NeRFs/DFANeRF/run_nerf_com_trainExpLater.py) on the synthetic dataset of
test_gpu_driver.py: rendering against the f32 tier's run, the range guard's refusal, training in the f32 tier and the
in-training preview's fallback."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from dfanerf import synth
from test_gpu_driver import COMMON, F_VAL, H, W, _run, dataset, t  # noqa: F401  (dataset: the module-scoped fixture)

pytestmark = pytest.mark.gpu

RENDER = "--render_person --test_file transforms_val_ba.json --N_rand=2048 --N_iters=600000 --image_ext png"
CKPT = "dataset/train_together/obama_TrainExpLater_smoMix/280000.tar"


def _frames(root, expname):
    from PIL import Image
    out = root / "dataset" / "train_together" / expname / "obama" / "person"
    return {sub: [np.asarray(Image.open(out / sub / f"test_{k:06d}.png").convert("RGB")).astype(int) for k in range(F_VAL)]
            for sub in ("render_com", "render_head")}


@pytest.fixture(scope="module")
def big_acts(dataset, states, latents):
    """a checkpoint whose head activations exceed half precision (test_gpu_driver.py: the f16 refusal test's)"""
    from dfanerf import nets, run_nerf
    from dfanerf.decoder import Decoder
    root, _ = dataset
    st = dict(states)
    st["decoder"] = synth.scale_head_activations(states["decoder"], 1.0e4)
    mods = {"decoder": Decoder(z_dim=256, hidden_size=256, dim_signal=96, use_deformation_field=True),
            "AudNet": nets.AudioNet_W2L(), "ExpNet": nets.ExpressionEnc(), "AudAttNet": nets.AudioAttNet(96, 4),
            "PoseAttNet": nets.AudioAttNet(42, 8)}
    for k, m in mods.items():
        m.load_state_dict({kk: t(v) for kk, v in st[k].items()})
    opts = {k: torch.optim.Adam(m.parameters(), lr=5e-4) for k, m in mods.items()}
    ck = root / "dataset" / "train_together" / "x3_big_acts"
    ck.mkdir(parents=True, exist_ok=True)
    run_nerf.save_checkpoint(str(ck / "280000.tar"), 280000, t(latents[0]), t(latents[1]), mods, opts)
    return "dataset/train_together/x3_big_acts/280000.tar"


def test_render_person_cli_f16x3_matches_the_f32_run(dataset):
    """the same --render_person run in both tiers: every frame's u8 images within one level of the f32 tier's"""
    root, _ = dataset
    _run(root, RENDER + f" --hip_tier f32 --expname x3_ref --resume {CKPT}")
    out = _run(root, RENDER + f" --hip_tier f16x3 --expname x3_run --resume {CKPT}")
    assert "f16x3 tier: calibrated on" in out and "max |activation|" in out
    ref, got = _frames(root, "x3_ref"), _frames(root, "x3_run")
    for sub in ref:
        for k in range(F_VAL):
            d = np.abs(got[sub][k] - ref[sub][k])
            print(f"{sub} frame {k}: {(d > 0).mean() * 100:.3f} % of the values differ, max {d.max()}")
            assert d.max() <= 1, (sub, k)


def test_f16x3_refuses_an_out_of_range_checkpoint_and_names_the_f32_tier(dataset, big_acts):
    root, _ = dataset
    cmd = [sys.executable, os.path.join(ROOT, "NeRFs", "DFANeRF", "run_nerf_com_trainExpLater.py")] + \
        (COMMON + " " + RENDER + f" --hip_tier f16x3 --expname x3_big --resume {big_acts}").split()
    r = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "F16RangeError" in r.stderr and "--hip_tier f16x3" in r.stderr and \
        "--hip_tier f32" in r.stderr, r.stderr[-1500:]
    res = root / "dataset" / "train_together" / "x3_big" / "obama" / "person" / "render_com"
    assert not res.exists() or not os.listdir(res)


@pytest.mark.parametrize("big", [False, True])
def test_f16x3_trains_in_f32_and_its_preview_falls_back(dataset, big_acts, big):
    """--hip_tier f16x3 in a training run: the step runs in the f32 tier; the periodic preview render is range-checked in
    f16x3 and, on a checkpoint half precision cannot hold, rendered in f32 with a warning instead of ending the run"""
    from PIL import Image
    root, _ = dataset
    name = "x3_train_big" if big else "x3_train"
    out = _run(root, "--N_rand=256 --N_iters=280002 --i_weights=100000 --i_test_person=280002 --image_ext png --hip_tier f16x3 "
                     f"--expname {name} --resume {big_acts if big else CKPT}")
    assert "--hip_tier f16x3: the training step runs in the f32 tier" in out
    if big:
        assert "WARNING: --hip_tier f16x3 refused for this preview, rendering it in the exact tier (f32)" in out
    else:
        assert "f16x3 tier: calibrated on" in out and "refused for this preview" not in out
    tdir = root / "dataset" / "train_together" / name / "obama" / "person" / "test_280002"
    assert sorted(os.listdir(tdir)) == ["test_000.png", "test_head_000.png"]
    assert np.asarray(Image.open(tdir / "test_000.png")).shape == (H, 2 * W, 3)
