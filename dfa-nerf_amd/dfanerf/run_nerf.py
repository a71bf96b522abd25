"""Host-side mirror of the reference driver run_nerf_com_trainExpLater.py: same CLI, same function names,
same dataset / checkpoint formats; the renderer behind them is the fused HIP kernel.

Reference: /root/reference/NeRFs/DFANeRF/run_nerf_com_trainExpLater.py (MAIN below).
  config_parser  MAIN:235-436 (all flags accepted; configargparse replaced by a small argparse subclass)
  encode_signal* MAIN:28-111          rot_to_euler / pose_to_euler_trans / euler2rot  MAIN:182-232
  composite_function MAIN:146-166     calc_volume_weights MAIN:169-179
  render_rays    MAIN:114-143 is dead upstream (TypeError at :138); here it works, with the semantics of the
                 live inline renderer MAIN:653-709 for one field
  train          MAIN:439-1246: render-person loop :590-734 -> FrameRenderer (one fused launch per frame
                 instead of 99 chunks x ~80 ATen launches); training loop :737-941; periodic test :943-1077;
                 LR schedule :1079-1094 (optimizer_Exp is never rescheduled - kept); checkpoints :1099-1117.
  run_network / create_nerf: names the task's north star asks for; thin shims (no upstream semantics exist).
Fixes relative to upstream: rot_to_euler uses the input's device instead of a
hard-coded .cuda(); the in-place `sigma[-1,:,:,-1] += 1e-6` on a relu output (rejected by current autograd) is
formed out of place; --render_final_video (broken upstream: .reshape on a list, MAIN:1163) uses the
render-person path."""
import argparse
import json
import math
import os
import time

import numpy as np
import torch

from . import parallel
from .decoder import Decoder
from .helpers import (AudioAttNet, AudioNet_W2L, ExpressionEnc, get_embedder, get_rays, img2mse, mse2psnr, sample_pdf,
                      to8b)
from .nets import encode_signal, encode_signal_torso, pose_to_euler_trans, rot_to_euler  # noqa: F401

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


# ------------------------------------------------------------------------------------------------------------
# CLI
# ------------------------------------------------------------------------------------------------------------
class ConfigArgParser(argparse.ArgumentParser):
    """argparse + `--config file` of `key = value` lines (what configargparse gives the reference):
    file values act as defaults, explicit command-line flags win.
    side: an optional second parser of store_true switches (config_parser: _OUTPUT_FLAGS); its flags are taken off the command
    line first and land in the same namespace."""
    side = None

    def format_help(self):
        return super().format_help() + ("\n" + self.side.format_help() if self.side is not None else "")

    def parse_args(self, args=None, namespace=None):
        import sys
        argv = list(sys.argv[1:] if args is None else args)
        if self.side is not None:
            side_ns, argv = self.side.parse_known_args(argv)
            namespace = namespace if namespace is not None else argparse.Namespace()
            for k, v in vars(side_ns).items():
                setattr(namespace, k, v)
        pre = argparse.ArgumentParser(add_help=False)
        pre.add_argument('--config')
        known, _ = pre.parse_known_args(argv)
        file_args = []
        if known.config:
            actions = {a.dest: a for a in self._actions}
            with open(known.config) as f:
                for line in f:
                    line = line.split('#')[0].strip()
                    if not line or '=' not in line:
                        continue
                    key, val = [s.strip() for s in line.split('=', 1)]
                    act = actions.get(key)
                    if act is None:
                        continue
                    if act.nargs == 0:
                        if val.lower() in ('true', '1', 'yes'):
                            file_args.append('--' + key)
                    else:
                        file_args += ['--' + key, val]
        return super().parse_args(file_args + argv, namespace)


# (flag, type, default) ; type None = store_true, 'sf' = store_false (quirk kept: --use_viewdirs, --no_batching
# and --white_bkgd are store_false upstream)
_FLAGS = [
    ("expname", str, None), ("basedir", str, './logs/'), ("datadir", str, './data/llff/fern'),
    ("netdepth", int, 8), ("netwidth", int, 256), ("netdepth_fine", int, 8), ("netwidth_fine", int, 256),
    ("N_rand", int, 2048), ("lrate", float, 5e-4), ("lrate_decay", int, 500), ("chunk", int, 4096),
    ("netchunk", int, 1024 * 64), ("no_batching", 'sf', None), ("no_reload", None, None), ("ft_path", str, None),
    ("N_iters", int, 400000), ("N_samples", int, 64), ("N_importance", int, 128), ("perturb", float, 1.),
    ("use_viewdirs", 'sf', None), ("i_embed", int, 0), ("multires", int, 10), ("multires_views", int, 4),
    ("raw_noise_std", float, 0.), ("render_only", None, None), ("render_test", None, None),
    ("render_factor", int, 0), ("precrop_iters", int, 0), ("precrop_frac", float, .5),
    ("dataset_type", str, 'audface'), ("testskip", int, 1), ("shape", str, 'greek'), ("white_bkgd", 'sf', None),
    ("half_res", None, None), ("with_test", int, 0), ("dim_aud", int, 64), ("sample_rate", float, 0.95),
    ("near", float, 0.3), ("far", float, 0.9), ("test_file", str, ''), ("aud_file", str, 'aud.npy'),
    ("exp_file", str, 'exp.pt'), ("win_size", int, 16), ("smo_size", int, 8), ("smo_torse_size", int, 4),
    ("nosmo_iters", int, 300000), ("noexp_iters", int, 300000), ("factor", int, 8), ("no_ndc", None, None),
    ("lindisp", None, None), ("spherify", None, None), ("llffhold", int, 8), ("i_print", int, 100),
    ("i_img", int, 500), ("i_weights", int, 10000), ("i_video", int, 50000), ("z_dim", int, 256),
    ("n_feat", int, 256), ("image_size", int, 256), ("n_object", int, 2), ("use_giraffe", None, None),
    ("resume", str, None), ("render_video", None, None), ("render_together", None, None),
    ("alpha_sigma_loss", float, None), ("concate_bg_render", None, None), ("concate_bg", None, None),
    ("stride", int, 2), ("render_person", None, None), ("i_test_separate", int, 1000), ("i_test_person", int, 1000),
    ("train_together", None, None), ("train_separate", None, None), ("dim_signal", int, 128),
    ("last_dist", float, 1e10), ("use_deformation_field", None, None), ("use_expression", None, None),
    ("use_et_embed", None, None), ("use_ba", None, None), ("render_final_video", None, None), ("no_com", None, None),
    ("use_L1", None, None), ("all_speaker", None, None), ("sample_rate_mouth", float, 0.7), ("use_exp", None, None),
    ("use_aud_net", None, None), ("use_ori", None, None), ("test_offset", int, 0),
]
# build-side additions (not in the reference): precision tier of the HIP renderer and the hierarchical mode
# --hip_tier: f32 (exact, the parity tier; default) | f16 (the throughput tier: f16 MFMA operands, PSNR-gated) | bf16
# (the 16-bit TRAINING tier; also selected for the training step when --hip_tier f16) | f16x3 (split f16 operands: the f32
# tier's accuracy at about a third of its time, range-guarded like f16; trains in f32)
# --image_ext: file type of the rendered frames (upstream writes .jpg, MAIN:722-732; png = the kernel's uint8 output
# losslessly, which is what the parity tests read back)
# --hip_train_act: format of the activations the 16-bit training step records for its weight gradients (fp4 | e4m3)
# --hip_f16_model_psnr: the model's PSNR against ground truth, for the f16 tier's accuracy guard where the frames being rendered
# have no ground truth (f16guard.py)
# --save_alpha / --save_depth: next to every rendered frame its opacity (alpha matte) and its expected depth, from the same launch
# (dfn_render_fwd_u8_aux)
_EXTRA_FLAGS = [("hip_tier", str, 'f32'), ("hierarchical", None, None), ("image_ext", str, 'jpg'), ("hip_train_act", str, 'fp4'),
                ("hip_f16_model_psnr", float, 30.0)]
# switches of what the render paths WRITE next to the frames (store_true; help in the table below).  They are parsed by a side
# parser (ConfigArgParser.side): the flag table proper stays the reference's flags plus the build-side switches above
_OUTPUT_FLAGS = ("save_alpha", "save_depth")
_EXTRA_HELP = {
    "hip_tier": "precision tier of the HIP path: f32 (exact MFMA products, the parity tier; default) | f16 (throughput tier "
                "for rendering: f16 MFMA operands, f32 accumulation) | f16x3 (rendering with the f32 tier's accuracy at about 3x "
                "its speed: every operand split into two f16 values, three f16 MFMAs per product; f16's range - a checkpoint "
                "outside it is refused, dfanerf/f16guard.py; trains in f32) | bf16.  TRAINING with f16 or bf16 runs the 16-bit "
                "training tier: bf16 MFMA operands in the forward and the dX chain, and the arrays recorded for the backward "
                "in MX block formats (one power-of-two scale per 64 features x 32 points): the pre-activation gradients as "
                "MX-fp8 (e4m3; values below amax * 2^-17 of a block flush to zero), the layer inputs as MX-fp4 (e2m1: ONE "
                "mantissa bit; --hip_train_act e4m3 records them in 8 bits instead) - the weight-gradient GEMMs run on them.  "
                "Use f32 for a reference-exact training run.  auto: render in f16 when the checkpoint passes the f16 tier's range "
                "AND accuracy guards on a calibration sample of the frames (dfanerf/f16guard.py), in f32 otherwise; trains in f32",
    "hip_f16_model_psnr": "f16 tier's accuracy guard: PSNR (dB) of the model against ground truth, used where the rendered frames "
                          "have none (with ground truth it is measured); the f16 image must stay within 0.05 dB of it",
    "hip_train_act": "16-bit training tier: format of the recorded layer inputs that feed the weight gradients: fp4 (MX-fp4 "
                     "e2m1, default: half the bytes; a weight gradient sums >= 131,072 points and the rounding averages out - "
                     "tests/test_gpu_convergence.py trains to convergence in both) | e4m3 (MX-fp8, +5 % step time)",
    "hierarchical": "N_samples + N_importance samples per ray (coarse pass -> sample_pdf -> the same decoder on the merged depths): "
                    "64 + 64 | 128; with --render_person also 32 + 32, 32 + 64 and 64 + 32 (the speed / quality knob of a render)",
    "image_ext": "file type of the rendered frames (jpg as upstream; png keeps the kernel's uint8 output losslessly)",
    "save_alpha": "write, next to every rendered frame <name>.<ext>, <name>_alpha.png: the opacity of the rendered foreground (alpha "
                  "matte of the head in render_head/, of head + torso in render_com/; background plane excluded) as 8-bit greyscale, "
                  "255 * acc truncated.  Always PNG.  --render_person and --render_final_video; the in-training preview ignores it; "
                  "one rank only (the per-frame gather carries RGB); tiers f32 / f16 / f16x3",
    "save_depth": "write <name>_depth.png next to every rendered frame: the expected depth of the foreground, PREMULTIPLIED by the "
                  "opacity (sum of weight * z over the foreground samples; divide by alpha for a mean depth), as 16-bit greyscale "
                  "(PIL mode I;16), 65535 * depth / far truncated.  Otherwise as --save_alpha",
}


def config_parser():
    parser = ConfigArgParser()
    parser.add_argument('--config', help='config file path')
    for name, typ, default in _FLAGS + _EXTRA_FLAGS:
        kw = {"help": _EXTRA_HELP[name]} if name in _EXTRA_HELP else {}
        if typ is None:
            parser.add_argument('--' + name, action='store_true', **kw)
        elif typ == 'sf':
            parser.add_argument('--' + name, action='store_false', **kw)
        else:
            parser.add_argument('--' + name, type=typ, default=default, **kw)
    parser.side = argparse.ArgumentParser(add_help=False, allow_abbrev=False, usage=argparse.SUPPRESS)
    grp = parser.side.add_argument_group("what the render paths write next to every frame (this build)")
    for name in _OUTPUT_FLAGS:
        grp.add_argument('--' + name, action='store_true', help=_EXTRA_HELP[name])
    return parser


def parse_config_file(config_path):
    with open(config_path, "r") as f:
        lines = f.readlines()
    return float(lines[3].split("=")[-1].strip()), float(lines[4].split("=")[-1].strip())


def euler2rot(euler_angle):
    """Batched XYZ euler -> rotation (MAIN:207-232; unused by the driver, kept for API parity)."""
    b = euler_angle.shape[0]
    th, ph, ps = [euler_angle[:, k].reshape(-1, 1, 1) for k in range(3)]
    one = torch.ones((b, 1, 1), dtype=torch.float32, device=euler_angle.device)
    zero = torch.zeros_like(one)
    rx = torch.cat((torch.cat((one, zero, zero), 1), torch.cat((zero, th.cos(), th.sin()), 1),
                    torch.cat((zero, -th.sin(), th.cos()), 1)), 2)
    ry = torch.cat((torch.cat((ph.cos(), zero, -ph.sin()), 1), torch.cat((zero, one, zero), 1),
                    torch.cat((ph.sin(), zero, ph.cos()), 1)), 2)
    rz = torch.cat((torch.cat((ps.cos(), -ps.sin(), zero), 1), torch.cat((ps.sin(), ps.cos(), zero), 1),
                    torch.cat((zero, zero, one), 1)), 2)
    return torch.bmm(rx, torch.bmm(ry, rz))


# ------------------------------------------------------------------------------------------------------------
# compositing API
# ------------------------------------------------------------------------------------------------------------
def _need_device(name, *tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{name} runs the HIP kernel and needs device tensors (there is no CPU fallback)")


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def composite_function(sigma, feat):
    """sigma [K,B,R,S], feat [K,B,R,S,3] -> sigma_sum [B,R,S], feat_weighted [B,R,S,3]  (MAIN:146-166).  dfn_composite; under
    autograd (a reference-shaped training loop, MAIN:888-889) an autograd node with dfn_composite_grad as its backward.  The
    production training step differentiates the fused renderer instead (training.FusedTrainFn)."""
    _need_device("composite_function", sigma, feat)
    from . import engine
    if _wants_grad(sigma, feat):
        from .training import CompositeFn
        return CompositeFn.apply(sigma, feat)
    return engine.composite(sigma.detach(), feat.detach())


def calc_volume_weights(z_vals, ray_vector, sigma, last_dist=1e10):
    """z [B,R,S], ray_vector [B,R,3], sigma [B,R,S] -> weights [B,R,S]  (MAIN:169-179).  dfn_volume_weights; under autograd an
    autograd node with dfn_volume_weights_grad as its backward (gradient of sigma: depths and ray vectors are constants of
    the training loop, MAIN:838-841 - a gradient request for them is refused rather than silently dropped)."""
    _need_device("calc_volume_weights", z_vals, ray_vector, sigma)
    from . import engine
    if _wants_grad(z_vals, ray_vector):
        raise RuntimeError("calc_volume_weights: gradients of z_vals / ray_vector are not implemented (constants of the "
                           "training loop, MAIN:838-841); detach them")
    if _wants_grad(sigma):
        from .training import VolumeWeightsFn
        return VolumeWeightsFn.apply(z_vals, ray_vector, sigma, last_dist)
    return engine.volume_weights(z_vals.detach(), ray_vector.detach(), sigma.detach(), last_dist)


def render_rays(decoder, p_i, r_i, z_shape_i, z_app_i, signal, head_or_torso, batch_size, bc_rgb, view_dir, z_vals,
                args, coarse_or_fine='coarse', raw_noise_std=0):
    """One field through decoder -> bg / sigma fix-ups -> composite -> weights -> (rgb, weights)   (MAIN:114-143; dead
    upstream - TypeError at :138 - here with the semantics of the live inline renderer MAIN:653-709 for one field).
    p_i, r_i [B, R*S, 3]; bc_rgb [B,R,1,3]; view_dir [B,R,3]; z_vals [B,R,S].  Every stage is a HIP launch (dfn_decoder_fwd,
    dfn_composite, dfn_volume_weights); when the decoder's parameters or the signals require grad and grad mode is on, the
    same stages run as autograd nodes (training.DecoderTrainFn, CompositeFn, VolumeWeightsFn): a reference-shaped loop
    can back-propagate a loss on the returned rgb.  The production training step is the fused renderer (training.render_train)."""
    S = args.N_samples + (args.N_importance if coarse_or_fine == 'fine' else 0)
    sigs = [s for s in (signal if isinstance(signal, (list, tuple)) else [signal]) if isinstance(s, torch.Tensor)]
    grad = torch.is_grad_enabled() and (any(s.requires_grad for s in sigs) or
                                        any(p.requires_grad for p in decoder.parameters()))
    with torch.enable_grad() if grad else torch.no_grad():
        feat_i, sigma_i = decoder(p_i, r_i, z_shape_i, z_app_i, signal, head_or_torso)
        sigma_i = sigma_i.reshape(batch_size, -1, S)
        feat_i = feat_i.reshape(batch_size, -1, S, 3)
        if args.concate_bg:
            feat_i = torch.cat((feat_i[..., :-1, :], bc_rgb.to(feat_i)), dim=-2)          # MAIN:669-671
        sigma = torch.clamp_min(sigma_i, 0.0)                                              # MAIN:688 F.relu
        if args.concate_bg:
            # MAIN:692-694, out of place (the in-place form on a ReLU output is rejected by autograd's version check)
            sigma = torch.cat((sigma[..., :-1], sigma[..., -1:] + 1e-6), dim=-1)
        sigma_sum, feat_weighted = composite_function(sigma.unsqueeze(0), feat_i.unsqueeze(0))
        weights = calc_volume_weights(z_vals, view_dir, sigma_sum, last_dist=args.last_dist)
        rgb = torch.sum(weights.unsqueeze(-1) * feat_weighted, dim=-2).squeeze(0)          # MAIN:706
    return rgb, weights


# ------------------------------------------------------------------------------------------------------------
# the fused renderer behind the frame loops
# ------------------------------------------------------------------------------------------------------------
def _host(pose):
    """3x4 pose as host numpy (the DfnFrame travels in the kernel arguments); a device tensor costs one sync."""
    if isinstance(pose, torch.Tensor):
        return pose.detach().cpu().numpy()
    return np.asarray(pose)


class _FrameWriter:
    """Output stage of the render loop (MAIN:712-732): the uint8 images leave the GPU through a small ring of pinned
    host buffers (asynchronous copy + event) and are JPEG-encoded on worker threads while the next frames render.
    Round 4: a POOL of encoder threads (PIL releases the GIL inside the encoder): one thread sustains ~110 frame pairs per
    second at 450 x 450 - enough next to one GPU's 14-45 frames/s, not next to eight - and the frames kept for the
    video are stored by sequence number, so their order does not depend on which thread finishes first.  stats(): how busy
    the encoders were and how long submit() had to wait for a free slot (the loop is output-bound when that is not ~0)."""

    def __init__(self, H, W, n_images, depth=None, workers=3):
        from concurrent.futures import ThreadPoolExecutor
        import time
        self._time = time.perf_counter
        self.workers = max(1, int(workers))
        depth = depth or (self.workers + 2)
        self.pool = ThreadPoolExecutor(max_workers=self.workers)
        self.cuda = torch.cuda.is_available()
        self.ring = [[torch.empty(H, W, 3, dtype=torch.uint8, pin_memory=self.cuda) for _ in range(n_images)]
                     for _ in range(depth)]
        self.pending = [None] * depth
        self.xring = {}                                      # slot -> pinned buffers of the extra planes (submit)
        self.k = 0
        self._kept = {}
        self._keep_list = None
        self._flushed = 0
        self.busy_s, self.blocked_s, self.t0 = 0.0, 0.0, None
        import threading
        self._lock = threading.Lock()                        # _kept / busy_s are touched by the worker threads

    def _flush_kept(self):
        # hand the kept frames to the caller's list in submission order, as far as they are complete
        # (frames submitted without a keep list leave a None marker: it advances the sequence and is not appended)
        while self._keep_list is not None and self._flushed in self._kept:
            a = self._kept.pop(self._flushed)
            if a is not None:
                self._keep_list.append(a)
            self._flushed += 1

    def submit(self, images, paths, keep=None, extras=()):
        """images: uint8 device tensors [H,W,3]; paths: file per image (None = do not write).
        extras: (device tensor [H,W] uint8 / uint16, path) pairs written as greyscale PNG by the same worker (--save_alpha /
        --save_depth); their pinned buffers join the slot's ring on first use."""
        if self.t0 is None:
            self.t0 = self._time()
        slot = self.k % len(self.ring)
        seq = self.k
        self.k += 1
        if self.pending[slot] is not None:
            t = self._time()
            self.pending[slot].result()                      # the slot's previous frame is on disk
            self.blocked_s += self._time() - t
        if keep is not None:
            self._keep_list = keep
        elif self._keep_list is None:
            self._flushed = self.k                           # nothing is kept for this frame: the sequence starts behind it
        with self._lock:
            self._flush_kept()
        bufs = self.ring[slot]
        for b, img in zip(bufs, images):
            b.copy_(img, non_blocking=True)
        extras = [(t, pth) for t, pth in extras if t is not None and pth]
        xb = self.xring.setdefault(slot, [])
        for i, (t, _) in enumerate(extras):
            if i >= len(xb) or xb[i].dtype != t.dtype or xb[i].shape != t.shape:
                xb[i:i + 1] = [torch.empty(t.shape, dtype=t.dtype, pin_memory=self.cuda)]
            xb[i].copy_(t, non_blocking=True)
        ev = None
        if self.cuda:
            ev = torch.cuda.Event()
            ev.record()

        def work():
            if ev is not None:
                ev.synchronize()
            t = self._time()
            arrs = [b.numpy().copy() for b in bufs[:len(images)]]
            for a, pth in zip(arrs, paths):
                if pth:
                    _imwrite(pth, a)
            for b, (_, pth) in zip(xb, extras):
                _imwrite_gray(pth, b.numpy())
            dt = self._time() - t
            with self._lock:
                # a marker per frame only while a keep list is active (it keeps the sequence gap-free for _flush_kept);
                # with keep=None throughout nothing is stored at all
                if keep is not None:
                    self._kept[seq] = arrs[0]
                elif self._keep_list is not None:
                    self._kept[seq] = None
                self.busy_s += dt
        self.pending[slot] = self.pool.submit(work)

    def drain(self):
        for f in self.pending:
            if f is not None:
                f.result()
        self.pending = [None] * len(self.pending)
        with self._lock:
            if self._keep_list is None:
                self._kept.clear()
                self._flushed = self.k
            self._flush_kept()

    def stats(self):
        wall = (self._time() - self.t0) if self.t0 is not None else 0.0
        # submit_waited_s: time submit() spent waiting for its slot's previous frame to be written - that wait INCLUDES the
        # frame's render (the worker first waits for the GPU event), so it is ~wall in a GPU-bound loop; the loop is
        # output-bound when encoder_utilisation approaches 1
        return {"frames": self.k, "workers": self.workers, "wall_s": wall, "encoder_busy_s": self.busy_s,
                "encoder_utilisation": self.busy_s / (wall * self.workers) if wall > 0 else 0.0,
                "submit_waited_s": self.blocked_s}


_AUX_RANKS_MSG = ("--save_alpha / --save_depth need a single rank: the per-frame gather across the ranks carries the RGB images only "
                  "(widening it is not implemented); render with one process, or drop the flags")


class FrameRenderer:
    """Replaces the chunked frame loop (MAIN:633-715): one fused launch per frame (per rank)."""

    def __init__(self, decoder, z_shape, z_app, bc_img, hwfcxy, near, far, args, itr_obj=0, tier=None):
        from . import engine
        self.engine = engine
        self.decoder, self.args = decoder, args
        self.tier = tier or getattr(args, "hip_tier", "f32")
        self.requested = self.tier
        # auto: f16 where the checkpoint passes both guards of the f16 tier (check_f16), the exact tier otherwise
        self.auto = self.tier == "auto"
        if self.auto:
            self.tier = "f16"
        H, W, focal, cx, cy = hwfcxy
        self.H, self.W, self.focal, self.cx, self.cy = int(H), int(W), float(focal), float(cx), float(cy)
        self.near, self.far = float(near), float(far)
        dev = next(decoder.parameters()).device
        self.bg = bc_img.reshape(-1, 3).to(dev).float().contiguous()          # [H*W,3] in [0,1]
        self.zs = z_shape[0, 2 * itr_obj:2 * itr_obj + 2].to(dev).float().contiguous()
        self.za = z_app[0, 2 * itr_obj:2 * itr_obj + 2].to(dev).float().contiguous()
        self.n_fine = args.N_importance if getattr(args, "hierarchical", False) else 0
        # --save_alpha / --save_depth: what render_image_begin(aux=True) asks the kernel for next to the uint8 images
        self.save_alpha, self.save_depth = bool(getattr(args, "save_alpha", False)), bool(getattr(args, "save_depth", False))

    @property
    def guarded(self):
        """the tier renders f16 operands (f16, f16x3, or auto): check_f16 belongs in front of its render loops"""
        return self.auto or self.requested in ("f16", "f16x3")

    def check_f16_range(self, poses, pose_body, signals, max_frames=8, n_rays=256):
        """f16 and f16x3 tiers only (no-op otherwise): calibrate the decoder's activation range on up to `max_frames` of the frames about
        to be rendered - poses[k] (3x4 host), signals(k) -> (sig_head [96], sig_torso [42]) - in the exact tier, and refuse
        (f16guard.F16RangeError) if half precision cannot hold it with margin: the f16 conversions do not saturate, an
        out-of-range checkpoint would render NaN silently.  The bounds stay on the packed decoder (`f16_bounds`)."""
        if self.tier not in ("f16", "f16x3") or len(poses) == 0:
            return None
        from . import f16guard
        pk = self.decoder.packed(self.tier)                 # (its weight bound was checked when it was packed)
        pick = sorted(set(np.linspace(0, len(poses) - 1, min(max_frames, len(poses))).astype(int).tolist()))
        frs, sh, stt = [], [], []
        for k in pick:
            a, b = signals(k)
            sh.append(a.reshape(-1))
            stt.append(b.reshape(-1))
            frs.append(self.engine.make_frame(self.H, self.W, self.focal, self.cx, self.cy, _host(poses[k]), _host(pose_body),
                                              self.near, self.far, self.args.last_dist, 0, n_rays, self.args.N_samples, 0, 2,
                                              self.args.concate_bg))
        with torch.no_grad():
            pk.f16_bounds = f16guard.activation_bounds(pk.flat, frs, sh, stt, self.zs, self.za, self.bg, n_rays=n_rays,
                                                       n_fine=self.n_fine, z_dim=pk.z_dim)
        top = f16guard.check(pk.f16_bounds, pk.f16_weight_max, tier=self.tier)
        print(f"[dfanerf] {self.tier} tier: calibrated on {len(pick)} frames x {n_rays} rays in the exact tier: max |activation| "
              f"{top:.4g}, max |parameter| {pk.f16_weight_max:.4g} (half precision holds {f16guard.F16_MAX:.0f}; margin x{f16guard.MARGIN:g})")
        return pk.f16_bounds

    def check_f16_accuracy(self, poses, pose_body, signals, max_frames=8, n_rays=256, targets=None, model_psnr=None, seed=0):
        """f16 tier only (no-op otherwise): the accuracy guard.  Renders `n_rays` random pixels of up to `max_frames` of the
        frames about to be rendered in the f16 tier AND in the exact tier, with the production settings (both fields, this
        renderer's n_fine, the frames' own poses and signals), and refuses (f16guard.F16AccuracyError) if the f16 images sit
        under the PSNR the north star's clause needs (f16guard.psnr_gate).  targets(k) -> (head [H*W,3], com [H*W,3]) ground
        truth (uint8 or float in [0,1], either may be None) where it exists: the model's own PSNR is then measured on the
        sample; model_psnr (dB) otherwise.  The statistics stay on the packed decoder (`f16_accuracy`)."""
        if self.tier != "f16" or len(poses) == 0:
            return None
        from . import f16guard
        eng, dev = self.engine, self.bg.device
        pick = sorted(set(np.linspace(0, len(poses) - 1, min(max_frames, len(poses))).astype(int).tolist()))
        gen = torch.Generator(device="cpu").manual_seed(seed)
        blocks = []
        with torch.no_grad():
            for k in pick:
                a, b = signals(k)
                pix = torch.randperm(self.H * self.W, generator=gen)[:n_rays].to(torch.int32).to(dev)
                img = {}
                for tier in ("f16", "f32"):
                    pk = self.decoder.packed(tier)
                    bias = pk.fold(a.reshape(-1), b.reshape(-1), self.zs, self.za)
                    fr = eng.make_frame(self.H, self.W, self.focal, self.cx, self.cy, _host(poses[k]), _host(pose_body), self.near,
                                        self.far, self.args.last_dist, 0, n_rays, self.args.N_samples, self.n_fine, 2,
                                        self.args.concate_bg)
                    img[tier] = eng.render(pk, bias, fr, self.bg, pix_index=pix)
                gt = targets(k) if targets is not None else (None, None)
                def at(t):
                    if t is None:
                        return None
                    t = torch.as_tensor(t).reshape(-1, 3).to(dev)[pix.long()]
                    return t.float() / 255.0 if t.dtype == torch.uint8 else t.float()
                blocks.append({"head": (img["f16"][0], img["f32"][0], at(gt[0])), "com": (img["f16"][1], img["f32"][1], at(gt[1]))})
        pk = self.decoder.packed("f16")
        pk.f16_accuracy = f16guard.accuracy_stats(blocks)
        mp = getattr(self.args, "hip_f16_model_psnr", None) if model_psnr is None else model_psnr
        gates = f16guard.check_accuracy(pk.f16_accuracy, mp)
        print("[dfanerf] f16 tier: accuracy on %d frames x %d rays against the exact tier: " % (len(pick), n_rays) +
              ", ".join(f"{n} {st['psnr_db']:.1f} dB (worst frame {st['worst_block_db']:.1f}, gate {gates[n]:.1f})"
                        for n, st in pk.f16_accuracy.items()))
        return pk.f16_accuracy

    def check_f16(self, poses, pose_body, signals, targets=None, max_frames=8, n_rays=256, fallback=False):
        """Both guards of the f16 tier in front of a render loop (no-op in any other tier): range, then accuracy.  With
        --hip_tier auto a refusal switches this renderer to the exact tier instead of raising.  The f16x3 tier has the range
        guard only (it keeps the f32 tier's accuracy); fallback=True (the in-training preview) renders in the exact tier with
        a warning when it refuses instead of raising.  -> the tier that will render."""
        if self.auto:
            self.tier = "f16"          # (every call decides again: the weights may have changed since the last one)
        elif self.requested == "f16x3":
            self.tier = "f16x3"
        if self.tier not in ("f16", "f16x3"):
            return self.tier
        from . import f16guard
        try:
            self.check_f16_range(poses, pose_body, signals, max_frames, n_rays)
            if self.tier == "f16":
                self.check_f16_accuracy(poses, pose_body, signals, max_frames, n_rays, targets=targets)
        except (f16guard.F16RangeError, f16guard.F16AccuracyError) as e:
            if self.auto:
                print(f"[dfanerf] --hip_tier auto: rendering in the exact tier (f32): {e}")
            elif fallback and self.tier == "f16x3":
                print(f"[dfanerf] WARNING: --hip_tier f16x3 refused for this preview, rendering it in the exact tier (f32): {e}")
            else:
                raise
            self.tier = "f32"
        return self.tier

    def render(self, pose, pose_body, signal, signal_torso, ray_begin=0, ray_count=None, pix_index=None, fields=2,
               out_u8=False, out=None, bias=None, want_alpha=False, want_depth=False):
        """-> rgb_head [n,3], rgb_com [n,3] (None if fields == 1); out_u8: uint8 images, to8b fused into the kernel;
        out: (head, com) tensors the kernel writes into (e.g. slices of the shard that is gathered); bias: the frame's folded
        bias blob if the caller already has it (engine.FramePrefetcher), instead of the two signals.
        want_alpha / want_depth (with out_u8): engine.render_u8's extra outputs follow, in its order."""
        eng = self.engine
        pk = self.decoder.packed(self.tier)
        if bias is None:
            bias = pk.fold(signal[0] if isinstance(signal, (list, tuple)) else signal,
                           signal_torso if fields == 2 else None, self.zs, self.za)
        n = (self.H * self.W - ray_begin) if ray_count is None else ray_count
        if pix_index is not None:
            n = pix_index.numel()
        fr = eng.make_frame(self.H, self.W, self.focal, self.cx, self.cy, _host(pose), _host(pose_body), self.near,
                            self.far, self.args.last_dist, ray_begin, n, self.args.N_samples, self.n_fine, fields,
                            self.args.concate_bg)
        oh, oc = out if out is not None else (None, None)
        if (want_alpha or want_depth) and not out_u8:
            raise ValueError("FrameRenderer.render: want_alpha / want_depth belong to the uint8 route (out_u8=True); "
                             "engine.render(want_aux=True) returns the float values")
        if out_u8:
            return eng.render_u8(pk, bias, fr, self.bg, pix_index=pix_index, out_head=oh, out_com=oc, want_alpha=want_alpha,
                                 want_depth=want_depth)
        return eng.render(pk, bias, fr, self.bg, pix_index=pix_index, out_head=oh, out_com=oc)

    def render_rays(self, rays_head, rays_torso, signal, signal_torso, bg, bounds=None, fields=2, out_u8=False, out=None,
                    bias=None):
        """render() for rays the caller supplies (engine.render(rays=): dfn_render_rays_fwd) - what a reference-shaped loop has
        after get_rays / ndc_rays, sub-pixel offsets, a lens model, or rays of several cameras concatenated.
        rays_head / rays_torso: (o, d) tensor pairs [..., 3] of the head field's and the torso field's rays (rays_torso is not
        used with fields == 1 and may be None); directions of any length.  bg: [R, 3] float in [0, 1] or uint8, row r the
        background of ray r (this renderer's own plate is indexed by pixel and is not used).  bounds: optional [R, 2] =
        (near, far) per ray; otherwise this renderer's near / far hold for every ray.  The run's tier and width,
        args.N_samples / n_fine / last_dist / concate_bg, out_u8, out and bias as in render().
        The f16 guards (check_f16) are NOT re-run here: they calibrate on the pinhole rays of the frames' poses, and rays that
        leave the volume those rays cover are the caller's to check (f16guard) before rendering them in the f16 / f16x3 tier.
        -> rgb_head [R,3], rgb_com [R,3] (None if fields == 1)."""
        eng = self.engine
        pk = self.decoder.packed(self.tier)
        if bias is None:
            bias = pk.fold(signal[0] if isinstance(signal, (list, tuple)) else signal,
                           signal_torso if fields == 2 else None, self.zs, self.za)
        if fields == 2 and rays_torso is None:
            raise ValueError("FrameRenderer.render_rays: fields == 2 needs rays_torso = (o, d)")
        rays = eng.pack_rays(rays_head[0], rays_head[1], *(rays_torso if fields == 2 else ()))
        n = rays.shape[0]
        dev = self.bg.device
        bg = torch.as_tensor(bg).to(dev).reshape(-1, 3)
        bg = (bg if bg.dtype == torch.uint8 else bg.float()).contiguous()
        # (H, W, the intrinsics, the poses and ray_begin are ignored by a rays launch)
        eye = np.eye(4, dtype=np.float32)
        fr = eng.make_frame(self.H, self.W, self.focal, self.cx, self.cy, eye, eye, self.near, self.far, self.args.last_dist, 0, n,
                            self.args.N_samples, self.n_fine, fields, self.args.concate_bg)
        oh, oc = out if out is not None else (None, None)
        if out_u8:
            return eng.render_u8(pk, bias, fr, bg, out_head=oh, out_com=oc, rays=rays.to(dev), bounds=bounds)
        return eng.render(pk, bias, fr, bg, out_head=oh, out_com=oc, rays=rays.to(dev), bounds=bounds)

    def render_image_begin(self, pose, pose_body, signal, signal_torso, fields=2, out_u8=False, bias=None, aux=False):
        """Start a whole frame: render this rank's ray shard and ISSUE the gather (async_op=True: it runs on the backend's
        own stream) -> a handle for render_image_end().  Two sets of shard / gather buffers alternate, so the gather of
        frame k runs underneath the render of frame k + 1: call begin(k + 1) before end(k).  ONE
        collective per frame: the kernel writes both images into one padded [n_img, per, 3] shard.
        aux: also what --save_alpha / --save_depth select (render_image_aux(handle) returns it); one rank only - the gather
        carries RGB."""
        import torch.distributed as dist
        R = self.H * self.W
        aux = bool(aux) and (self.save_alpha or self.save_depth)
        if not (dist.is_initialized() and dist.get_world_size() > 1):
            if aux:
                res = self.render(pose, pose_body, signal, signal_torso, fields=fields, out_u8=out_u8, bias=bias,
                                  want_alpha=self.save_alpha, want_depth=self.save_depth)
                planes = {}
                if self.save_alpha:
                    planes["alpha_head"], planes["alpha_com"] = res[2:4]
                if self.save_depth:
                    planes["depth_head"], planes["depth_com"] = res[-2:]
                return {"images": res[:2], "aux": planes}
            rh, rc = self.render(pose, pose_body, signal, signal_torso, fields=fields, out_u8=out_u8, bias=bias)
            return {"images": (rh, rc)}
        if aux:
            raise RuntimeError(_AUX_RANKS_MSG)
        world = dist.get_world_size()
        begin, count, per = parallel.shard_range(R, world, dist.get_rank())
        n_img = 2 if fields == 2 else 1
        key = (n_img, per, out_u8, world)
        if getattr(self, "_shard_key", None) != key:
            dt = torch.uint8 if out_u8 else torch.float32
            self._slots = [{"shard": torch.zeros(n_img, per, 3, dtype=dt, device=self.bg.device),
                            "gathered": torch.empty(world, n_img, per, 3, dtype=dt, device=self.bg.device), "work": None}
                           for _ in range(2)]
            self._flip, self._shard_key = 0, key
            # Consecutive frames alternate between TWO render streams (one per buffer set): a rank's shard is 12.4 rounds of
            # workgroups at 8 ranks, and on one stream the 13th, partial round leaves 64 % of the compute units idle (5 % of
            # the frame) - the next frame's workgroups, launched on the other stream, start on them (measured on one GPU,
            # tools/shard_scaling.py --two-streams: a 1/8 shard 4.09 -> 3.90 ms per frame = 95.6 % -> 100 % of linear)
            self._rstreams = [self.engine.side_stream(self.bg.device, role="render_a"),
                              self.engine.side_stream(self.bg.device, role="render_b")]
        self._flip ^= 1
        slot = self._slots[self._flip]
        rs = self._rstreams[self._flip]
        rs.wait_stream(torch.cuda.current_stream(self.bg.device))      # pose-independent inputs (signals / blob) of the caller
        with torch.cuda.stream(rs):
            if slot["work"] is not None:               # the frame that used these buffers two frames ago was never finished
                slot["work"].wait()
                slot["work"] = None
            shard = slot["shard"]
            out = (shard[0, :count], shard[1, :count] if fields == 2 else None)
            if count:
                self.render(pose, pose_body, signal, signal_torso, begin, count, fields=fields, out_u8=out_u8, out=out,
                            bias=bias)
            # the output as the CONCATENATION of the shards along dim 0 (the stacked [world, ...] form is an NCCL / RCCL
            # extension that gloo rejects)
            slot["work"] = dist.all_gather_into_tensor(slot["gathered"].view(world * n_img, per, 3), shard, async_op=True)
        # "stream": what read the caller's inputs (engine.FramePrefetcher.done() must record its event there)
        return {"slot": slot, "n_img": n_img, "per": per, "world": world, "fields": fields, "stream": rs}

    def render_image_end(self, h):
        """Finish a frame started by render_image_begin: order the current stream behind its gather -> [H,W,3] images
        (views of the gather buffer: valid until the second render_image_begin after this frame's)."""
        R = self.H * self.W
        if "images" in h:
            rh, rc = h["images"]
        else:
            slot = h["slot"]
            if slot["work"] is not None:
                slot["work"].wait()
                slot["work"] = None
            g = slot["gathered"].permute(1, 0, 2, 3).reshape(h["n_img"], h["world"] * h["per"], 3)[:, :R]
            rh, rc = g[0], (g[1] if h["fields"] == 2 else None)
        return rh.reshape(self.H, self.W, 3), (rc.reshape(self.H, self.W, 3) if rc is not None else None)

    def render_image_aux(self, h):
        """The aux planes of a frame started with render_image_begin(aux=True): {"alpha_head", "alpha_com"} uint8 [H,W] and /
        or {"depth_head", "depth_com"} uint16 [H,W] (the _com entries None with one field); {} when none were asked for."""
        return {k: (v.reshape(self.H, self.W) if v is not None else None) for k, v in h.get("aux", {}).items()}

    def render_image(self, pose, pose_body, signal, signal_torso, fields=2, out_u8=False):
        """Whole frame, sharded over the ranks when torch.distributed is initialised -> [H,W,3] images
        (float32, or uint8 with out_u8: 76 KB instead of 304 KB per rank in the gather).  begin + end in one call; the
        frame loops call the two halves themselves to overlap a frame's gather with the next frame's render."""
        return self.render_image_end(self.render_image_begin(pose, pose_body, signal, signal_torso, fields, out_u8))


def run_network(inputs, viewdirs, decoder, z_shape, z_app, signal, head_or_torso='head'):
    """North-star shim: evaluate the decoder at points `inputs` [..., 3] with directions `viewdirs` [..., 3]."""
    feat, sigma = decoder(inputs.reshape(1, -1, 3), viewdirs.reshape(1, -1, 3), z_shape, z_app, signal, head_or_torso)
    return feat.reshape(*inputs.shape[:-1], 3), sigma.reshape(inputs.shape[:-1])


def make_adam(params, lr):
    """torch.optim.Adam(lr, betas=(0.9, 0.999)) as upstream (MAIN:522-547), as optim.HipAdam: the same optimizer (update
    rule, state_dict layout) with step() as one dfn_adam_multi launch per distinct step count - torch's fused
    multi-tensor kernel takes 104 us for the decoder's 68 tensors, the five optimizers 250 us of a 2.9 ms step.

    The gradient guard (grad_guard_env: DFN_GRAD_GUARD / DFN_MAX_GRAD_NORM in the environment) goes to EVERY optimizer made
    here: each of the five networks is guarded on its own stream, over its own parameters.  One norm across the five would
    need a join of their streams in front of the first update - the join the step's schedule was built to avoid (DESIGN.md
    section 5, LABNOTES section 7)."""
    params = list(params)
    if not params or not all(p.is_cuda for p in params):
        raise RuntimeError("make_adam: the parameters must live on the GPU (HipAdam; there is no CPU path)")
    from .optim import HipAdam
    return HipAdam(params, lr=lr, betas=(0.9, 0.999), **grad_guard_env())


def grad_guard_env(env=None):
    """HipAdam's guard arguments from the environment (the command-line flag tables are fixed; DFN_WIDTH is the precedent):
    DFN_GRAD_GUARD=1 skips a step whose gradients hold a NaN or an Inf, DFN_MAX_GRAD_NORM=<float> clips the total norm.
    Both unset (or empty): {} - the unguarded step.  A value that does not parse is an error here, at start-up."""
    env = os.environ if env is None else env
    out = {}
    g = str(env.get("DFN_GRAD_GUARD", "")).strip()
    if g not in ("", "0", "1"):
        raise ValueError(f"DFN_GRAD_GUARD={g!r}: 1 (skip steps with non-finite gradients) or 0 / unset")
    if g == "1":
        out["skip_nonfinite"] = True
    m = str(env.get("DFN_MAX_GRAD_NORM", "")).strip()
    if m:
        try:
            v = float(m)
        except ValueError:
            raise ValueError(f"DFN_MAX_GRAD_NORM={m!r}: a finite number >= 0 (the bound on the total gradient norm)") from None
        if not math.isfinite(v) or v < 0:
            raise ValueError(f"DFN_MAX_GRAD_NORM={m!r}: a finite number >= 0 (the bound on the total gradient norm)")
        out["max_grad_norm"] = v
    return out


def create_nerf(args, dev=None):
    """North-star shim: build the networks and optimizers exactly as train() does (MAIN:512-547)."""
    dev = dev or device
    embed_fn, dim_torso_signal = None, None
    if args.use_et_embed:
        embed_fn, input_ch = get_embedder(3, 0)
        dim_torso_signal = 2 * input_ch
    nets = {"decoder": Decoder(z_dim=args.z_dim, hidden_size=args.n_feat, dim_signal=args.dim_signal,
                               use_deformation_field=args.use_deformation_field,
                               use_expression=args.use_expression, use_aud_net=args.use_aud_net).to(dev),
            "AudNet": AudioNet_W2L().to(dev), "ExpNet": ExpressionEnc().to(dev),
            "AudAttNet": AudioAttNet(dim_aud=args.dim_aud, seq_len=args.smo_size).to(dev)}
    if args.use_et_embed:
        nets["PoseAttNet"] = AudioAttNet(dim_aud=dim_torso_signal, seq_len=args.smo_torse_size).to(dev)
    opts = {k: make_adam(m.parameters(), args.lrate) for k, m in nets.items()}
    return nets, opts, embed_fn


# checkpoint layout (MAIN:1101-1115)
_CKPT_NET = {"decoder": "network_decoder_state_dict", "AudNet": "network_AudNet_state_dict",
             "ExpNet": "network_ExpNet_state_dict", "AudAttNet": "network_AudAttNet_state_dict",
             "PoseAttNet": "network_PoseAttNet_state_dict"}
_CKPT_OPT = {"decoder": "optimizer_decoder_state_dict", "AudNet": "optimizer_Aud_state_dict",
             "ExpNet": "optimizer_Exp_state_dict", "AudAttNet": "optimizer_AudAtt_state_dict",
             "PoseAttNet": "optimizer_PoseAtt_state_dict"}


# key order of the dict upstream saves (MAIN:1101-1115; golden G12 pins it)
_CKPT_ORDER = [("net", "decoder"), ("net", "AudNet"), ("net", "ExpNet"), ("opt", "decoder"), ("opt", "AudNet"),
               ("opt", "ExpNet"), ("net", "AudAttNet"), ("opt", "AudAttNet"), ("net", "PoseAttNet"), ("opt", "PoseAttNet")]


def save_checkpoint(path, global_step, z_shape, z_app, nets, opts):
    ck = {'global_step': global_step, 'z_shape': z_shape, 'z_app': z_app}
    for kind, k in _CKPT_ORDER:
        if k in nets:
            if kind == "net":
                ck[_CKPT_NET[k]] = nets[k].state_dict()
            else:
                ck[_CKPT_OPT[k]] = opts[k].state_dict()
    torch.save(ck, path)


def load_checkpoint(path, nets, opts, map_location=None):
    """MAIN:553-580: decoder + its optimizer are mandatory, the rest optional."""
    ck = torch.load(path, map_location=map_location, weights_only=False)
    nets["decoder"].load_state_dict(ck[_CKPT_NET["decoder"]])
    opts["decoder"].load_state_dict(ck[_CKPT_OPT["decoder"]])
    for k in nets:
        if k != "decoder" and _CKPT_NET[k] in ck:
            nets[k].load_state_dict(ck[_CKPT_NET[k]])
        if k != "decoder" and _CKPT_OPT[k] in ck:
            opts[k].load_state_dict(ck[_CKPT_OPT[k]])
    return ck['global_step'], ck['z_shape'], ck['z_app']


def _imread(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def _imwrite(path, arr):
    from PIL import Image
    Image.fromarray(np.asarray(arr, np.uint8)).save(path, quality=95)


def _imwrite_gray(path, arr):
    """[H,W] uint8 -> 8-bit greyscale PNG (mode L); uint16 -> 16-bit greyscale PNG (mode I;16)"""
    from PIL import Image
    a = np.ascontiguousarray(arr)
    if a.dtype == np.uint16:
        Image.frombytes('I;16', (a.shape[1], a.shape[0]), a.astype('<u2').tobytes()).save(path, format='PNG')
    else:
        Image.frombytes('L', (a.shape[1], a.shape[0]), a.astype(np.uint8).tobytes()).save(path, format='PNG')


def _mimwrite(path, frames, fps=25):
    try:
        import imageio
        imageio.mimwrite(path, frames, fps=fps, quality=8)
        return True
    except Exception as e:       # imageio / ffmpeg are not part of this image
        print(f'[dfanerf] video not written ({e.__class__.__name__}: {e}); frames are saved as jpg')
        return False


def _choice_distinct(rng, n, k):
    """k distinct indices of range(n), uniform over the k-subsets, in random order - what
    np.random.choice(n, k, replace=False) gives upstream (MAIN:818-820), but O(k) instead of a permutation of all n
    (2.9 ms per step for n = 202,500: it was the longest host-side item of the training step)."""
    if k * 4 >= n:
        return rng.choice(n, size=[k], replace=False)
    got = np.unique(rng.randint(0, n, size=k + k // 4 + 16))
    while got.shape[0] < k:
        got = np.unique(np.concatenate([got, rng.randint(0, n, size=k)]))
    return got[rng.permutation(got.shape[0])[:k]]


def select_coords(H, W, N_rand, sample_rate, rect, rng=np.random):
    """Pixel sampling of MAIN:786-820 on the host (np.random as upstream); returns int64 [N_rand, 2] (y, x)."""
    if sample_rate > 0:
        # rect_num pixels from (face rect | lower half), the rest from outside (MAIN:786-817): rejection sampling on
        # uniform distinct candidates, classified arithmetically (no H*W meshgrid / nonzero per step)
        def inside(p):
            y, x = p // W, p % W
            in_rect = (y >= rect[0]) & (y <= rect[0] + rect[2]) & (x >= rect[1]) & (x <= rect[1] + rect[3])
            return in_rect | (y >= H / 2)
        rect_num = int(N_rand * sample_rate)
        need = {True: rect_num, False: N_rand - rect_num}
        have = {True: np.empty(0, np.int64), False: np.empty(0, np.int64)}
        tries = 0
        while any(have[c].shape[0] < need[c] for c in (True, False)):
            cand = _choice_distinct(rng, H * W, min(H * W, 4 * N_rand << min(tries, 4)))
            m = inside(cand)
            for c in (True, False):
                if have[c].shape[0] < need[c]:
                    have[c] = np.unique(np.concatenate([have[c], cand[m == c]]))
            tries += 1
            if tries > 64:
                raise ValueError("select_coords: not enough pixels inside / outside the sampling region")
        sel = np.concatenate([have[c][rng.permutation(have[c].shape[0])[:need[c]]] for c in (True, False)])
    else:
        sel = _choice_distinct(rng, H * W, N_rand)
    return np.stack([sel // W, sel % W], 1).astype(np.int64)


def train_step_loss_hip(nets, dataset, itr_obj, img_i, sel_yx, target_head, target_com, z_shape, z_app, global_step,
                        args, len_train, embed_fn, pose_torso, buf):
    """Forward of one training step (MAIN:779-907) with the decoder forward+backward, ray generation, sampling and
    compositing in the fused HIP kernels (training.FusedTrainFn).  `buf`: training.TrainBuffers for len(sel_yx) rays.
    sel_yx: [n,2] (y, x) pixel coordinates (numpy or device tensor) or an int32 device tensor [n] of pixel ids y*W+x
    (frames.PixelSampler).  target_head / target_com: float [n,3] targets, or the whole uint8 ground-truth frames
    [H*W,3] on the device (frames.DeviceFrameCache) - then the loss kernel gathers the targets itself."""
    from . import engine, training
    dec = nets["decoder"]
    dev = next(dec.parameters()).device
    poses = dataset[itr_obj]['poses']
    H, W, focal, cx, cy = dataset[itr_obj]['hwfcxy']
    H, W = int(H), int(W)
    sig_tr = getattr(buf, "signal_trainer", None)
    if sig_tr is not None and itr_obj == 0:
        # rows A7 / A8 forward + backward in HIP (training.SignalTrainer): 4 launches instead of ~200
        smoothed = global_step >= args.nosmo_iters
        s2, t2 = sig_tr.encode(img_i, args.smo_size if smoothed else 0, args.smo_torse_size if smoothed else 0, len_train)
        signal, signal_torso = [s2, None], t2         # [1,42] as it comes (an index op here would put an autograd node
                                                      # between the two HIP Functions, see training.render_train)
    else:
        signal = encode_signal(dataset, itr_obj, img_i, args.dim_aud, nets["AudNet"], nets["ExpNet"], nets["AudAttNet"],
                               global_step, args, len_train, embed_fn=embed_fn)
        signal_torso = encode_signal_torso(dataset, itr_obj, img_i, nets.get("PoseAttNet"), global_step, args,
                                           len_train, embed_fn=embed_fn)
    if isinstance(sel_yx, torch.Tensor) and sel_yx.dim() == 1:
        pix = sel_yx.to(device=dev, dtype=torch.int32)
    elif isinstance(sel_yx, torch.Tensor):
        pix = (sel_yx[:, 0] * W + sel_yx[:, 1]).to(device=dev, dtype=torch.int32)
    else:
        if getattr(buf, "upload", None) is None:
            buf.upload = training.PinnedUpload()
        pix = buf.upload(np.asarray(sel_yx[:, 0] * W + sel_yx[:, 1], dtype=np.int32), torch.int32, dev)
    # the frame geometry travels in the kernel arguments: keep host copies of the poses (a .cpu() per step would
    # synchronise the stream and serialise the host with the previous step's kernels)
    d = dataset[itr_obj]
    if d.get('_poses_host_of') is not poses:
        d['_poses_host'], d['_poses_host_of'] = poses.detach().cpu().numpy(), poses
    if isinstance(pose_torso, torch.Tensor):
        key = (pose_torso.data_ptr(), pose_torso._version)
        if d.get('_pose_torso_key') != key:
            d['_pose_torso_host'], d['_pose_torso_key'] = pose_torso.detach().cpu().numpy(), key
        pose_torso = d['_pose_torso_host']
    # --hierarchical (build-side flag): the step differentiates row H (64 + N_importance samples, fine depths detached)
    frame = engine.make_frame(H, W, focal, cx, cy, d['_poses_host'][img_i], pose_torso, d['near'], d['far'],
                              args.last_dist, 0, pix.numel(), args.N_samples, buf.n_fine, 2, args.concate_bg)
    bg = dataset[itr_obj]['bc_img'].reshape(-1, 3)
    zs = z_shape[0, itr_obj * 2:itr_obj * 2 + 2]
    za = z_app[0, itr_obj * 2:itr_obj * 2 + 2]
    tr_arg = sig_tr if (sig_tr is not None and itr_obj == 0) else None
    if target_head.dtype == torch.uint8 and not args.use_L1:
        # the production step: forward + both losses + their sum as ONE autograd node (training.FusedTrainLossFn; start its
        # backward with training.backward(loss, buf) and no ATen kernel runs between the forward and the dX chain)
        return training.render_train_loss(dec, buf, frame, bg, pix, signal[0], signal_torso, zs, za, target_head, target_com,
                                          signal_trainer=tr_arg)
    rgb_head, rgb_com = training.render_train(dec, buf, frame, bg, pix, signal[0], signal_torso, zs, za, signal_trainer=tr_arg)
    if target_head.dtype == torch.uint8:
        # whole uint8 ground-truth frames [H*W,3] resident on the device (frames.DeviceFrameCache): the targets are gathered
        # inside the loss kernel (dfn_mse_loss_u8: MAIN:791-800 + 902-907 + their autograd in one launch)
        l_head, l_com = training.mse_losses(rgb_head, rgb_com, target_head, target_com, pix)
        if args.use_L1:
            target_com = target_com[pix.long()].float() / 255.0
    else:                                   # explicit float targets [n,3]
        l_head = img2mse(rgb_head, target_head)
        l_com = img2mse(rgb_com, target_com)
    loss = l_com + l_head
    if args.use_L1:
        # MAIN:909-912 as written upstream: the L1 term pairs the HEAD image with the composite target and replaces
        # the MSE sum; without --train_together upstream's loss is the integer 0 and backward() fails
        if not args.train_together:
            raise ValueError("--use_L1 needs --train_together (upstream's loss is the constant 0 otherwise, MAIN:909-912)")
        loss = torch.mean(torch.abs(rgb_head - target_com))
    return loss, l_head, l_com, rgb_head, rgb_com


def draw_stream(train_buf):
    """The side stream the pipelined pixel draw of the NEXT step runs on (frames.PixelSampler(pipeline=True, stream=...)): one of
    the process's four (a fifth stream shares a hardware queue with another one).  Round 4: the general side stream - the head
    field's weight gradients, idle from the middle of the backward on.  Until round 3 it was the pose network's stream, whose
    chain (backward -> Adam -> the next step's encoder) is the LAST thing a step waits for: the 20-us draw sat in front of the
    encoder forward the next step's decoder needs (DFN_DRAW_STREAM=pose restores that for A/B)."""
    import os
    tr = getattr(train_buf, "signal_trainer", None)
    if tr is None:
        return None
    if os.environ.get("DFN_DRAW_STREAM", "wgrad") == "pose":
        return tr.pose_stream()
    from . import engine
    return engine.side_stream(tr.device, role="wgrad")


def _hip_signals_ok(args):
    """The HIP signal encoders (dfn_encode_signal*) cover the reference configuration: 96-wide audio+expression signal,
    even attention windows up to 8 frames.  Anything else goes through the torch modules (nets.encode_signal*)."""
    ok = lambda n: 0 < n <= 8 and n % 2 == 0
    return args.dim_aud == 96 and ok(args.smo_size) and ok(args.smo_torse_size)


def optimizer_steps(opts, global_step, args):
    """Gating of MAIN:924-931.  (HipAdam.step_unhooked = step() without torch's per-call profiler / hook wrapper.)"""
    step = lambda o: getattr(o, "step_unhooked", o.step)()
    step(opts["decoder"])
    step(opts["AudNet"])
    if global_step >= args.nosmo_iters:
        step(opts["AudAttNet"])
        if args.use_et_embed and "PoseAttNet" in opts:
            step(opts["PoseAttNet"])
    if global_step >= args.noexp_iters:
        step(opts["ExpNet"])


def update_lrate(opts, global_step, args):
    """MAIN:1081-1094: exponential decay; x2 for the attention nets; optimizer_Exp is never touched."""
    new_lrate = args.lrate * (0.1 ** (global_step / (args.lrate_decay * 1500)))
    for k, mult in (("decoder", 1), ("AudNet", 1), ("AudAttNet", 2), ("PoseAttNet", 2)):
        if k in opts:
            for g in opts[k].param_groups:
                g['lr'] = new_lrate * mult
    return new_lrate


def check_supported(args):
    """The HIP path implements the configuration scripts/{train,test}_obama.sh build (LABNOTES.md section 1): say so when
    the arguments are parsed, not at the first kernel launch."""
    bad = []
    if args.dim_signal != 96:
        bad.append(f"--dim_signal {args.dim_signal} (supported: 96 - what the signal encoders emit, upstream too)")
    # --z_dim / --n_feat 1 ... 256 (upstream: free): a narrower network lives in the library's 256-wide layout with zero rows / columns -
    # the same function exactly, forward and backward (engine.flatten_state, training._FlatNet).  Inference of --n_feat <= 128 runs
    # natively on the 128-wide program (f32 / f16 / f16x3 tiers: Decoder.packed, engine.select_width); --n_feat 129 ... 255, the bf16
    # tier and every training step stay padded, at the 256-wide network's cost
    if not 0 < args.z_dim <= 256:
        bad.append(f"--z_dim {args.z_dim} (supported: 1 ... 256)")
    if not 0 < args.n_feat <= 256:
        bad.append(f"--n_feat {args.n_feat} (supported: 1 ... 256)")
    # (--use_expression: accepted - with one person the reference's decoder registers expnet and never evaluates it, MAIN:70)
    # (without --use_deformation_field, a store_true flag upstream: the fused torso program runs an all-zero deformation network that
    # nothing ever steps - deform(p) + p = p exactly)
    if args.N_samples not in (32, 64, 128):
        bad.append(f"--N_samples {args.N_samples} (supported: 32, 64, 128)")
    if getattr(args, "hierarchical", False):
        # the renderer's rule (include/dfanerf.h): one coarse sample per lane of the fine sampler's wave, N_importance <= 2 N_samples
        if args.N_samples not in (32, 64):
            bad.append(f"--hierarchical with --N_samples {args.N_samples} (the fused fine sampler works on 32 or 64 coarse samples)")
        elif args.N_importance not in (32, 64, 128) or args.N_importance > 2 * args.N_samples:
            bad.append(f"--hierarchical with --N_samples {args.N_samples} --N_importance {args.N_importance} (supported: N_importance "
                       "32, 64 or 128, at most 2 x N_samples)")
        elif not args.render_person and (args.N_samples != 64 or args.N_importance not in (64, 128)):
            bad.append(f"--hierarchical with --N_samples {args.N_samples} --N_importance {args.N_importance} in a training run (the "
                       "hierarchical training step is 64 + 64 | 128; the other counts render only: --render_person)")
    if args.n_object < 1:
        bad.append(f"--n_object {args.n_object}")
    # (--n_object > 1, the flag's default: accepted like upstream - and like upstream the run stops in the setup loop over the
    # persons, train(): the reference builds ONE dataset, `datadir = [args.datadir]` (MAIN:449), and indexes it per person)
    if args.hip_tier not in ("f32", "f16", "f16x3", "bf16", "auto"):
        bad.append(f"--hip_tier {args.hip_tier} (f32 | f16 | f16x3 | bf16 | auto)")
    if getattr(args, "hip_train_act", "fp4") not in ("fp4", "e4m3"):
        bad.append(f"--hip_train_act {args.hip_train_act} (fp4 | e4m3)")
    if (getattr(args, "save_alpha", False) or getattr(args, "save_depth", False)) and args.hip_tier == "bf16":
        bad.append("--save_alpha / --save_depth with --hip_tier bf16 (the opacity / depth outputs exist in the f32, f16 and f16x3 tiers)")
    if bad:
        raise SystemExit("run_nerf_com_trainExpLater.py (MI355X build): unsupported configuration:\n  " + "\n  ".join(bad))


def train():
    from .load_audface import load_audface_data_split
    args = config_parser().parse_args()
    check_supported(args)
    world, rank, local = parallel.init()
    want_aux = bool(getattr(args, "save_alpha", False) or getattr(args, "save_depth", False))
    if want_aux and world > 1:
        raise SystemExit("run_nerf_com_trainExpLater.py (MI355X build): " + _AUX_RANKS_MSG)
    dev = torch.device("cuda", local) if torch.cuda.is_available() else torch.device("cpu")
    if dev.type != "cuda":
        raise RuntimeError("train(): no HIP device visible; the render path has no CPU fallback")
    print("args.near: ", args.near)
    print("args.far: ", args.far)
    tf = 'transforms_train_ba.json' if args.use_ba else 'transforms_train.json'
    with open(os.path.join(args.datadir, tf), 'r') as fp:
        pose_body = torch.Tensor(json.load(fp)['frames'][0]['transform_matrix']).to(dev).float()
    ds = load_audface_data_split(args.datadir, args.testskip, test_file=args.test_file, aud_file=args.aud_file,
                                 exp_file=args.exp_file, no_com=args.no_com, all_speaker=args.all_speaker,
                                 use_ori=args.use_ori, use_ba=args.use_ba, test_offset=args.test_offset)
    ds['near'], ds['far'] = args.near, args.far
    if not args.render_person:
        ds['i_train'], ds['i_val'] = ds['i_split']
        ds['i_train'] = np.intersect1d(ds['i_train'], np.where(ds['speak_frames'] > 0))
    for k in ('poses', 'auds', 'exp'):
        ds[k] = torch.Tensor(ds[k]).to(dev).float()
    ds['bc_img'] = torch.Tensor(ds['bc_img']).to(dev).float() / 255.0
    datasets = [ds]
    batch_size = 1
    basedir = os.path.join('dataset/train_together', args.expname)
    # MAIN:449, 495-501: one output directory per person out of a ONE-element `datadir` list - with the flag's default
    # (--n_object 2) upstream stops right here with IndexError('list index out of range'); the scripts pass --n_object 1.
    # Reproduced as is: what a second person WOULD evaluate (the listener input layers, MAIN:72-75, decoder.py:306-307) exists
    # on this path - Decoder.forward(signal=[None, ...]) renders and trains in HIP (field 2) - but no dataset reaches it.
    datadir = [args.datadir]
    imgdir = []
    for k in range(args.n_object):
        if k >= len(datadir):      # the same exception at the same place as upstream, with the reason spelled out
            raise IndexError(f"list index out of range (--n_object {args.n_object}: like upstream, one dataset is loaded - datadir = "
                             "[args.datadir], MAIN:449 - and person %d has none; the scripts pass --n_object 1)" % k)
        i_dir = os.path.join(basedir, datadir[k].split('/')[-1])
        if rank == 0:
            os.makedirs(os.path.join(i_dir, 'person'), exist_ok=True)
        imgdir.append(i_dir)
    if rank == 0:
        with open(os.path.join(basedir, 'args.txt'), 'w') as f:
            for arg in sorted(vars(args)):
                f.write('{} = {}\n'.format(arg, getattr(args, arg)))
        if args.config is not None:
            with open(os.path.join(basedir, 'config.txt'), 'w') as f:
                f.write(open(args.config, 'r').read())
    nets, opts, embed_fn = create_nerf(args, dev)
    z_shape = torch.randn(batch_size, args.n_object * 2, args.z_dim).to(dev)
    z_app = torch.randn(batch_size, args.n_object * 2, args.z_dim).to(dev)
    global_step = 0
    if args.resume is not None:
        global_step, z_shape, z_app = load_checkpoint(args.resume, nets, opts, map_location=dev)
        z_shape, z_app = z_shape.to(dev), z_app.to(dev)
    if world > 1:
        # data-parallel replicas must start identical: every rank initialised its own networks and latents from its own
        # RNG (and only rank 0's are ever saved) - rank 0's parameters, buffers, Adam moments and latent codes go to all
        z_shape, z_app = parallel.broadcast_replicas(nets, opts, [z_shape, z_app], src=0)
    print('N_rand', args.N_rand, 'no_batching', args.no_batching, 'sample_rate', args.sample_rate)
    print('Begin')
    itr_obj = 0
    H, W, focal, cx, cy = ds['hwfcxy']
    H, W = int(H), int(W)
    renderer = FrameRenderer(nets["decoder"], z_shape, z_app, ds['bc_img'], ds['hwfcxy'], args.near, args.far, args)

    poses_host = ds['poses'][:, :3, :4].detach().cpu().numpy()       # one copy, no per-frame sync

    def render_frames(frame_ids, len_sig, outdir_com, outdir_head, pose_body_t, tag='test_{:06d}.jpg'):
        rgbs = []
        if args.image_ext != 'jpg':
            tag = tag[:-3] + args.image_ext
        writer = _FrameWriter(H, W, 2)
        body_host = _host(pose_body_t)
        # conditioning signals through the HIP encoders (dfn_encode_signal*, rows A7 / A8) when the whole path is on
        # the GPU with the reference's configuration (pose attention on); otherwise the torch modules
        enc = None
        if "PoseAttNet" in nets and embed_fn is not None and _hip_signals_ok(args):
            from . import engine
            enc = engine.SignalEncoder(nets["AudNet"], nets["ExpNet"], nets["AudAttNet"], nets["PoseAttNet"],
                                       ds['auds'], ds['exp'], ds['poses'])
        smoothed = global_step >= args.nosmo_iters
        def finish(handle, img_i):
            rgb8_head, rgb8 = renderer.render_image_end(handle)
            if rank == 0:
                # --save_alpha / --save_depth: <name>_alpha.png / <name>_depth.png next to each image's file
                planes = renderer.render_image_aux(handle)
                stem = os.path.splitext(tag.format(img_i))[0]
                extras = [(planes.get(kind + "_" + img), os.path.join(d, stem + "_" + kind + ".png") if d else None)
                          for kind in ("alpha", "depth") for img, d in (("com", outdir_com), ("head", outdir_head))]
                writer.submit([rgb8, rgb8_head],
                              [os.path.join(outdir_com, tag.format(img_i)),
                               os.path.join(outdir_head, tag.format(img_i)) if outdir_head else None], keep=rgbs, extras=extras)
                print('Saved test img at {}'.format(os.path.join(outdir_com, tag.format(img_i))))
        pending = None
        frame_ids = list(frame_ids)
        # the per-frame front end (signal encoders + bias fold) one frame ahead on a side stream (engine.FramePrefetcher)
        pf = None
        if enc is not None:
            pf = engine.FramePrefetcher(enc, renderer.decoder.packed(renderer.tier), renderer.zs, renderer.za,
                                        args.smo_size if smoothed else 0, args.smo_torse_size if smoothed else 0, fields=2,
                                        length=len_sig)
        if renderer.guarded and frame_ids:
            # range guard of the f16 tier (f16guard.py): a few hundred rays of up to eight of these frames through the exact
            # tier, with their own poses and signals; refuses a checkpoint whose activations half precision cannot hold
            def sig_of(k):
                img_i = frame_ids[k]
                if enc is not None:
                    s2, t2 = enc.encode([img_i], args.smo_size if smoothed else 0, args.smo_torse_size if smoothed else 0,
                                        length=len_sig)
                    return s2[0], t2[0]
                with torch.no_grad():
                    sg = encode_signal(datasets, itr_obj, img_i, args.dim_aud, nets["AudNet"], nets["ExpNet"], nets["AudAttNet"],
                                       global_step, args, len_sig, embed_fn=embed_fn)
                    st_ = encode_signal_torso(datasets, itr_obj, img_i, nets.get("PoseAttNet"), global_step, args, len_sig,
                                              embed_fn=embed_fn)
                return sg[0], st_
            # ... and the accuracy guard: the same sample in f16 AND the exact tier, production settings (f16guard.py, round 6)
            renderer.check_f16([poses_host[i] for i in frame_ids], body_host, sig_of)
            if pf is not None and pf.pk is not renderer.decoder.packed(renderer.tier):       # (auto fell back to the exact tier)
                pf = engine.FramePrefetcher(enc, renderer.decoder.packed(renderer.tier), renderer.zs, renderer.za,
                                            args.smo_size if smoothed else 0, args.smo_torse_size if smoothed else 0, fields=2,
                                            length=len_sig)
        for k, img_i in enumerate(frame_ids):
            with torch.no_grad():
                if pf is not None:
                    bias = pf.get(img_i, frame_ids[k + 1] if k + 1 < len(frame_ids) else None)
                    handle = renderer.render_image_begin(poses_host[img_i], body_host, None, None, out_u8=True, bias=bias,
                                                         aux=want_aux)
                    with torch.cuda.stream(handle.get("stream") or torch.cuda.current_stream(dev)):
                        pf.done()                       # (on the stream the render that read the blob runs on)
                    if pending is not None:
                        finish(*pending)
                    pending = (handle, img_i)
                    continue
                else:
                    signal = encode_signal(datasets, itr_obj, img_i, args.dim_aud, nets["AudNet"], nets["ExpNet"],
                                           nets["AudAttNet"], global_step, args, len_sig, embed_fn=embed_fn)
                    signal_torso = encode_signal_torso(datasets, itr_obj, img_i, nets.get("PoseAttNet"), global_step,
                                                       args, len_sig, embed_fn=embed_fn)
                # uint8 straight from the kernel epilogue (to8b fused), gathered as uint8 across the ranks; pipelined by one
                # frame: this frame's render is enqueued BEFORE the previous frame's gather is waited for
                handle = renderer.render_image_begin(poses_host[img_i], body_host, signal, signal_torso, out_u8=True, aux=want_aux)
                if pending is not None:
                    finish(*pending)
                pending = (handle, img_i)
        if pending is not None:
            finish(*pending)
        writer.drain()
        if rank == 0 and len(frame_ids) > 1:
            import json
            st_ = writer.stats()
            st_["frames_per_s"] = st_["frames"] / st_["wall_s"] if st_["wall_s"] > 0 else 0.0
            print('[dfanerf] render loop: ' + json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in st_.items()}))
        return rgbs

    if args.render_person:
        print('RENDER PERSON')
        out_com = os.path.join(imgdir[0], 'person', 'render_com')
        out_head = os.path.join(imgdir[0], 'person', 'render_head')
        if rank == 0:
            os.makedirs(out_com, exist_ok=True)
            os.makedirs(out_head, exist_ok=True)
        n_items = ds['auds'].shape[0]
        print("num_items: ", n_items)
        rgbs = render_frames(range(n_items), n_items, out_com, out_head, pose_body[:3, :4])
        if args.render_video and rank == 0:
            _mimwrite(os.path.join(out_com, '{}.mp4'.format(args.expname)), rgbs)
        return

    if want_aux and rank == 0:
        print("[dfanerf] --save_alpha / --save_depth: written for the rendered frames (--render_person, --render_final_video); the "
              "in-training preview ignores them")
    from . import training
    # the 16-bit training tier is bf16 (f16, the inference throughput tier, has too little exponent range for gradients)
    tier = getattr(args, "hip_tier", "f32")
    # (auto = the fastest tier that keeps the accuracy clause: training is exact; f16x3 asks for the f32 tier's numbers: so does its
    # training step)
    if tier == "f16x3":
        print("[dfanerf] --hip_tier f16x3: the training step runs in the f32 tier (f16x3 renders only)")
    tier = "f32" if tier in ("auto", "f16x3") else tier
    train_buf = training.TrainBuffers("bf16" if tier == "f16" else tier, args.N_rand, dev,
                                      n_fine=args.N_importance if getattr(args, "hierarchical", False) else 0,
                                      act_format=getattr(args, "hip_train_act", None), n_coarse=args.N_samples)
    if "PoseAttNet" in nets and _hip_signals_ok(args):
        train_buf.signal_trainer = training.SignalTrainer(nets["AudNet"], nets["ExpNet"], nets["AudAttNet"],
                                                          nets["PoseAttNet"], ds['auds'], ds['exp'], ds['poses'])
        train_buf.signal_trainer.adopt_optimizers(opts)
    bucket = parallel.StepReducer(nets, opts, getattr(train_buf, "signal_trainer", None)) if world > 1 else None
    rng = np.random.RandomState(1234 + rank) if world > 1 else np.random
    i_train = ds['i_train']
    # training input stage on the device: uint8 ground-truth frames resident in HBM (decoded
    # once; an LRU of decoded frames if the sequence does not fit), pixels drawn on the device, targets gathered inside
    # the loss kernel - upstream decodes two JPEGs and uploads two frames every step (MAIN:771-774, 791-800)
    from . import frames
    cache = frames.DeviceFrameCache(ds['imgs'], ds['imgs_com'], H, W, dev,
                                    budget_bytes=int(float(os.environ.get("DFN_FRAME_CACHE_GB", "32")) * (1 << 30)))
    if len(i_train) <= cache.capacity:
        t0 = time.time()
        n_pre = cache.preload(i_train, log=print if rank == 0 else None)
        if rank == 0:
            print(f'[dfanerf] {n_pre} ground-truth frame pairs decoded to the device in {time.time() - t0:.1f} s')
    sampler = frames.PixelSampler(H, W, args.N_rand, args.sample_rate, dev, seed=1234 + rank,
                                  rects=ds['sample_rects'] if args.sample_rate > 0 else None, pipeline=True,
                                  stream=draw_stream(train_buf))
    # the draw is a function of (seed, counter): continue the stream where the checkpoint left it, so that a resumed run
    # (scripts/train_obama.sh always resumes from 280000.tar) does not replay the pixel sequence of the run before it -
    # upstream draws from the unseeded global np.random.  Nothing extra is stored in the checkpoint.
    sampler.counter = int(global_step)
    from tqdm import trange, tqdm
    guard_on, guard_seen = getattr(opts["decoder"], "_guarded", False), 0
    for i in trange(global_step + 1, args.N_iters + 1, disable=rank != 0):
        img_i = rng.choice(i_train)
        pix = sampler.draw(frame=img_i if args.sample_rate > 0 else None)
        target_head_s, target_com_s = cache.get(img_i)
        loss, l_head, l_com, _, _ = train_step_loss_hip(nets, datasets, itr_obj, img_i, pix, target_head_s,
                                                        target_com_s, z_shape, z_app, global_step, args,
                                                        len(i_train), embed_fn, ds['poses'][0, :3, :4], train_buf)
        for o in opts.values():
            o.zero_grad()
        training.backward(loss, train_buf)          # loss.backward() with the buffers' own unit gradient (FusedTrainLossFn)
        if bucket is not None:
            bucket.all_reduce_()
        optimizer_steps(opts, global_step, args)
        if i % args.i_print == 0 and rank == 0:
            msg = (f"[TRAIN] Iter: {i} Object: {itr_obj} Com Loss: {l_com.item()}  Head Neck PSNR: "
                   f"{mse2psnr(l_head).item()} Com PSNR: {mse2psnr(l_com).item()}")
            tqdm.write(msg)
            with open(os.path.join(basedir, 'loss.txt'), 'a') as f:
                f.write(msg + "\n")
            if guard_on:        # (optim.HipAdam's gradient guard: a line of its own when steps were skipped since the last print)
                n_skip = opts["decoder"].grad_stats()["skipped_total"]
                if n_skip > guard_seen:
                    guard_seen = n_skip
                    msg = f"[GUARD] Iter: {i} Network: decoder Skipped steps (non-finite gradient): {n_skip}"
                    tqdm.write(msg)
                    with open(os.path.join(basedir, 'loss.txt'), 'a') as f:
                        f.write(msg + "\n")
        sig_tr = getattr(train_buf, "signal_trainer", None)
        if sig_tr is not None and ((i % args.i_test_person == 0 and i > 0) or i in [100, 500, 1000, 3000] or
                                   i % args.i_weights == 0):
            sig_tr.join()       # the conditioning networks' Adam runs on their own streams: order this one behind it
        if (i % args.i_test_person == 0 and i > 0) or (i in [100, 500, 1000, 3000]):
            # periodic test (MAIN:943-1077): every 100th validation frame, body pose = training frame 0; files
            # test_head_%03d / test_%03d (numbered by the position in i_val) hold render | ground truth side by side,
            # the PSNR is taken on the float composite image
            outdir = os.path.join(imgdir[0], 'person', 'test_{}'.format(i))
            if rank == 0:
                os.makedirs(outdir, exist_ok=True)
            i_val = ds['i_val']
            enc_t = None
            if "PoseAttNet" in nets and embed_fn is not None and _hip_signals_ok(args):
                from . import engine
                enc_t = engine.SignalEncoder(nets["AudNet"], nets["ExpNet"], nets["AudAttNet"], nets["PoseAttNet"],
                                             ds['auds'], ds['exp'], ds['poses'])
            smoothed = global_step >= args.nosmo_iters
            def test_signals(img_id):
                with torch.no_grad():
                    if enc_t is not None:
                        s2, t2 = enc_t.encode([img_id], args.smo_size if smoothed else 0,
                                              args.smo_torse_size if smoothed else 0, length=len(i_train) + len(i_val))
                        return s2[0], t2[0]
                    sg = encode_signal(datasets, itr_obj, img_id, args.dim_aud, nets["AudNet"], nets["ExpNet"], nets["AudAttNet"],
                                       global_step, args, len(i_train) + len(i_val), embed_fn=embed_fn)
                    st_ = encode_signal_torso(datasets, itr_obj, img_id, nets.get("PoseAttNet"), global_step, args,
                                              len(i_train) + len(i_val), embed_fn=embed_fn)
                    return sg[0], st_
            test_ids = [i_val[t] for t in range(0, len(i_val), 100)]
            if renderer.guarded and test_ids:
                # the weights change every step: both guards of the f16 tier again on the frames about to be rendered, the model's
                # own PSNR measured against their ground truth (this render used to run unguarded).  f16x3: a range
                # refusal renders this preview in f32 with a warning instead of ending the run
                renderer.check_f16([poses_host[j] for j in test_ids], poses_host[0], lambda k: test_signals(test_ids[k]),
                                   targets=lambda k: (_imread(ds['imgs'][test_ids[k]]), _imread(ds['imgs_com'][test_ids[k]])),
                                   fallback=True)
            for testimg_i in range(0, len(i_val), 100):
                img_id = i_val[testimg_i]
                with torch.no_grad():
                    if enc_t is not None:
                        s2, t2 = enc_t.encode([img_id], args.smo_size if smoothed else 0,
                                              args.smo_torse_size if smoothed else 0, length=len(i_train) + len(i_val))
                        signal, signal_torso = [s2, None], t2[0]
                    else:
                        signal = encode_signal(datasets, itr_obj, img_id, args.dim_aud, nets["AudNet"], nets["ExpNet"],
                                               nets["AudAttNet"], global_step, args, len(i_train) + len(i_val),
                                               embed_fn=embed_fn)
                        signal_torso = encode_signal_torso(datasets, itr_obj, img_id, nets.get("PoseAttNet"), global_step,
                                                           args, len(i_train) + len(i_val), embed_fn=embed_fn)
                    rgb_head, rgb = renderer.render_image(poses_host[img_id], poses_host[0], signal, signal_torso)
                if rank == 0:
                    ext = args.image_ext
                    for img, tgt_path, name in ((rgb_head, ds['imgs'][img_id], 'test_head_{:03d}.'.format(testimg_i) + ext),
                                                (rgb, ds['imgs_com'][img_id], 'test_{:03d}.'.format(testimg_i) + ext)):
                        target_img = _imread(tgt_path)
                        _imwrite(os.path.join(outdir, name), np.concatenate((to8b(img).cpu().numpy(), target_img), axis=1))
                    target_rgb = torch.as_tensor(target_img).to(dev).float() / 255.0
                    ps = mse2psnr(img2mse(rgb, target_rgb))
                    print('Saved test person img, psnr: {}'.format(ps.item()))
                    with open(os.path.join(basedir, 'loss.txt'), 'a') as f:
                        f.write(f"[TEST] Iter: {i} Object: {itr_obj}_person PSNR: {ps.item()}\n")
        update_lrate(opts, global_step, args)
        global_step += 1
        if i % args.i_weights == 0 and rank == 0:
            path = os.path.join(basedir, '{:06d}.tar'.format(i))
            save_checkpoint(path, global_step, z_shape, z_app, nets, opts)
            print('Saved checkpoints at', path)
    torch.cuda.synchronize()            # the loop never waits for the GPU: make sure the last steps have run before leaving
    if args.render_final_video:
        outdir = os.path.join(imgdir[0], 'person')
        rgbs = render_frames(list(ds['i_val']), len(ds['i_val']), outdir, None, pose_body[:3, :4],
                             tag='final_{:06d}.jpg')
        if rank == 0:
            _mimwrite(os.path.join(outdir, 'test_{}_{}.mp4'.format(args.N_iters, args.expname)), rgbs)


if __name__ == '__main__':
    train()
