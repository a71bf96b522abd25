#!/usr/bin/env python3
"""Write the fixtures of tests/test_gpu_f16_bits.py (tests/golden/f16_bits/*.npy) from the library in use: the plain f16 launches of
every case, two ray windows stacked on axis 0.  The fixtures in the tree were written ONCE, with the library of the commit before
LABNOTES.md 4.8 (DFN_LIB=<that library> python tools/f16_bits_dump.py); writing them again with a later library un-pins the f16
tier's bits, so do that only for a change that is MEANT to move them.

  python tools/f16_bits_dump.py [--out DIR]        (needs the GPU)
Prints, per case and window, what the rays see (largest foreground weight, spread of the image) and whether the rays / z / aux entry
points equal the plain launch with this library."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "dfa-nerf_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))
import test_gpu_f16_bits as T                                           # noqa: E402
from dfanerf import engine, synth                                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=T.FIX)
a = ap.parse_args()
engine.require_gpu()
os.makedirs(a.out, exist_ok=True)
golden = lambda name: dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))
world = T.World(engine, synth.bench_scene(0, n_frames=8), synth.synth_all_states(0), synth.synth_latents(0), golden)
for case in T.CASES:
    per = [world.plain(case, begin) for begin in T.WINDOWS]
    for k in per[0]:
        arr = torch.stack([p[k] for p in per]).numpy()
        assert arr.dtype == np.float32 and np.isfinite(arr).all()
        np.save(os.path.join(a.out, f"{T.case_name(*case)}_{k}.npy"), arr)
    for wi, begin in enumerate(T.WINDOWS):
        fix = per[wi]
        eq = {}
        for route in ("rays", "aux") + (("z",) if case[3] == 0 else ()):
            got = world.through(case, begin, route, fix["z"])
            eq[route] = all(torch.equal(v, fix[k]) for k, v in got.items())
        print(f"{T.case_name(*case):16s} window {wi}: max foreground w_head {float(fix['w_head'][:, :-1].max()):.3f}"
              + (f", w_com {float(fix['w_com'][:, :-1].max()):.3f}" if "w_com" in fix else "")
              + f", std rgb_head {float(fix['rgb_head'].std()):.3f}; equal to plain: {eq}", flush=True)
