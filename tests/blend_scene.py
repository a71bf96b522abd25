"""The BLEND decoder and what the tests on it share - TEST INFRASTRUCTURE ONLY (a plain helper module like tests/twins.py).

The fixtures' synthetic decoder (dfanerf.synth) gives the torso a raw density of up to 145 against the head's 32: every ray of the
two-field composite is opaque within a few samples, so the per-sample blend sigma = sigma_h + sigma_t, feat = (sigma_h feat_h +
sigma_t feat_t) / sigma is only ever exercised where one field swamps the other.  blend_state() is the same network with the torso's
two input matrices scaled by TORSO_SCALE and sigma_out.bias shifted by SIGMA_SHIFT: translucent composites, rays on which both
fields carry weight, importance samplers fed many different inverse CDFs, and a composite loss whose gradient reaches the deep
samples (tests/test_blend_scene_host.py asserts all of this with the CPU oracle).

Also here: the 93 rays of tests/test_gpu_samples.py, golden G7's conditioning, the oracle wrappers the GPU tests share (Oracle), and
the CPU model of what a 16-bit tier's operand rounding costs (rounder / posenc16 / model_fields: test_pack_plan.emulate with its
rounding hook on dense weights) from which tests/test_gpu_blend.py derives the 16-bit tiers' gates."""
import numpy as np
import torch

import dfa_oracle as O

TORSO_SCALE = 0.03
SIGMA_SHIFT = -18.0
N_RAYS = 93
FRAME = 2
TORSO_ONLY = ("deform_net.", "fc_in_torso.", "fc_p_skips_torso.")          # parameters only the torso field reads


def t(x):
    return torch.from_numpy(np.asarray(x))


def blend_state(states, torso_scale=TORSO_SCALE, sigma_shift=SIGMA_SHIFT):
    """a copy of states["decoder"] with fc_in_torso.weight and fc_p_skips_torso.0.weight scaled and sigma_out.bias shifted"""
    st = {k: np.array(v, copy=True) for k, v in states["decoder"].items()}
    for k in ("fc_in_torso.weight", "fc_p_skips_torso.0.weight"):
        st[k] = (st[k] * np.float32(torso_scale)).astype(np.float32)
    st["sigma_out.bias"] = (st["sigma_out.bias"] + np.float32(sigma_shift)).astype(np.float32)
    return st


def blend_states(states):
    """all five networks' states with the decoder replaced by the blend decoder"""
    out = dict(states)
    out["decoder"] = blend_state(states)
    return out


def ray_indices(scene, n_rays=N_RAYS):
    """a stride through the whole frame; 93 is no multiple of 4 or 8: the last workgroup has idle waves in every tier"""
    n = scene["H"] * scene["W"]
    idx = np.arange(11, n, n // n_rays)[:n_rays].astype(np.int32)
    assert len(idx) == n_rays
    return idx


def conditioning(g7, latents):
    """(sig_head [96], sig_torso [42], z_shape [2, 256], z_app [2, 256]) of golden g7_frame_coarse, as PackedDecoder.fold takes them"""
    return g7["signal"][0], g7["signal_torso"].reshape(-1), latents[0][0], latents[1][0]


class Oracle:
    """the CPU oracle on `pix` of frame FRAME for one decoder state: rays, conditioning and results computed once"""

    def __init__(self, scene, dec_state, latents, g7, pix=None, frame=FRAME):
        self.scene, self.state = scene, dec_state
        self.pix = ray_indices(scene) if pix is None else pix
        self.P = O.params_to_torch(dec_state)
        self.zs, self.za = [t(v) for v in latents]
        geo = (scene["H"], scene["W"], scene["focal"])
        o_h, d_h = O.get_rays(*geo, scene["poses"][frame][:3, :4], scene["cx"], scene["cy"])
        o_t, d_t = O.get_rays(*geo, scene["pose_body"][:3, :4], scene["cx"], scene["cy"])
        sel = t(self.pix).long()
        self.rays = [x.reshape(-1, 3)[sel].contiguous() for x in (o_h, d_h, o_t, d_t)]
        self.bg = (t(scene["bg"]).float() / 255.0).reshape(-1, 3)[sel]
        self.sig, self.sigt = [t(g7["signal"]), None], t(g7["signal_torso"])
        self.near, self.far = scene["near"], scene["far"]
        self._cache = {}

    def render(self, nc, nf, fields):
        """render_rays_chunk(..., return_aux=True) -> (rgb_head, rgb_com, aux), once per (n_coarse, n_fine, fields)"""
        key = (nc, nf, fields)
        if key not in self._cache:
            with torch.no_grad():
                self._cache[key] = O.render_rays_chunk(self.P, *self.rays, self.bg, self.near, self.far, self.zs, self.za, self.sig,
                                                       self.sigt, nc, nf, fields, return_aux=True)
        return self._cache[key]

    def fields_at(self, z, fields=2):
        """_eval_fields at depths z [n, S] -> sigma_h, feat_h, sigma_t, feat_t (raw densities)"""
        with torch.no_grad():
            return O._eval_fields(self.P, *self.rays, t(z), self.zs, self.za, self.sig, self.sigt, fields)

    def integrate(self, z, s_h, f_h, s_t, f_t):
        """integrate_fields -> rgb_head, w_head, rgb_com, w_com"""
        return O.integrate_fields(t(z), self.rays[1], self.rays[3], s_h, f_h, s_t, f_t, self.bg)

    def at(self, z, fields=2):
        """decoder + compositing at depths z -> rgb_head, w_head, rgb_com, w_com (what render_fixed_samples computes, with the weights)"""
        with torch.no_grad():
            return self.integrate(z, *self.fields_at(z, fields))


# ---- the reference's own float32 error ------------------------------------------------------------------------------------------
# max |w(float64 oracle) - w(float32 oracle)| over the 93 rays, any single weight, largest of the sample pairs (32, 0), (64, 0),
# (32, 32), (32, 64), (64, 128) at the oracle's own depths - measured with oracle_f64 below (both at 32 + 0; the other pairs:
# head 1.6e-6 ... 2.8e-6, com 1.1e-6 ... 1.6e-6).  The fixtures' decoder gives 2.7e-6 / 1.9e-6: its opaque composites hide nothing
# here, the project's 2e-6 per-weight gate was simply never held against more than golden G7's rays.
W_F64 = {"head": 5.04e-6, "com": 1.77e-6}


def oracle_f64(orc, z):
    """the oracle's own arithmetic in float64 at depths z: parameters, rays, depths and conditioning are the float32 values, cast;
    the encoding keeps the reference's float32 constants c_i = fl32(2^i pi) -> rgb_head, w_head, rgb_com, w_com (float64)"""
    import math
    keep = O.posenc

    def posenc_c32(p, n_freq, downscale=2.0):
        p = p / downscale
        out = []
        for i in range(n_freq):
            c = float(np.float32((2 ** i) * math.pi))
            out += [torch.sin(c * p), torch.cos(c * p)]
        return torch.cat(out, -1)
    O.posenc = posenc_c32
    try:
        with torch.no_grad():
            d = lambda x: None if x is None else x.double()
            P = {k: v.double() for k, v in orc.P.items()}
            rays = [d(r) for r in orc.rays]
            s = O._eval_fields(P, *rays, t(z).double(), d(orc.zs), d(orc.za), [d(orc.sig[0]), None], d(orc.sigt), 2)
            return O.integrate_fields(t(z).double(), rays[1], rays[3], *s, d(orc.bg))
    finally:
        O.posenc = keep


# ---- what the scene is like: the figures tests/test_blend_scene_host.py asserts ---------------------------------------------------
def scene_figures(orc, nc):
    """-> dict of the oracle's figures at nc coarse samples, two fields (numpy, per ray where it says so)"""
    _, _, aux = orc.render(nc, 32, 2)
    w_c, w_h = aux["w_com_coarse"].numpy().astype(np.float64), aux["w_head_coarse"].numpy().astype(np.float64)
    z = aux["z_coarse"]
    s_h, _, s_t, _ = orc.fields_at(z.numpy(), 2)
    rh, rt = np.maximum(s_h.numpy().astype(np.float64), 0), np.maximum(s_t.numpy().astype(np.float64), 0)
    fg = slice(0, nc - 1)                                          # concate_bg: the last sample is the background plane
    tot = rh[:, fg] + rt[:, fg]
    frac = np.where(tot > 0, rh[:, fg] / np.where(tot > 0, tot, 1.0), 0.0)
    share = (w_c[:, fg] * frac).sum(1) / np.maximum(w_c[:, fg].sum(1), 1e-300)
    return {"acc_com": w_c[:, fg].sum(1), "acc_head": w_h[:, fg].sum(1), "head_share": share,
            "argmax_bins": np.unique(w_c[:, 1:-1].argmax(1)), "z_fine": aux["z_fine"].numpy()}


def deep_gradient_share(orc, nc=64, first=4, seed=0):
    """share of |d rgb_com / d sigma_h| and |d rgb_com / d sigma_t| (autograd through integrate_fields, a fixed random d_rgb_com)
    that lies behind the first `first` samples"""
    z = O.coarse_z(orc.near, orc.far, nc)[None].expand(len(orc.pix), nc).contiguous()
    s_h, f_h, s_t, f_t = orc.fields_at(z.numpy(), 2)
    s_h, s_t = s_h.clone().requires_grad_(True), s_t.clone().requires_grad_(True)
    _, _, rgb_c, _ = orc.integrate(z.numpy(), s_h, f_h, s_t, f_t)
    d = torch.randn(rgb_c.shape, generator=torch.Generator().manual_seed(seed))
    (rgb_c * d).sum().backward()
    out = []
    for g in (s_h.grad, s_t.grad):
        a = g.abs().double()
        out.append(float(a[:, first:].sum() / a.sum()))
    return tuple(out)


# ---- the rounding model of the 16-bit tiers ------------------------------------------------------------------------------------
def _bf16(x, toward_zero):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    if not toward_zero:
        b = b + 0x7FFF + ((b >> 16) & 1)                            # nearest, ties to even
    return (b & 0xFFFF0000).astype(np.uint32).view(np.float32).astype(np.float64)


def _f16(x, toward_zero):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):                                 # beyond 65504: inf, as v_cvt_pk_f16_f32 gives
        r = x.astype(np.float16)                                    # nearest, ties to even (one rounding from float64)
    if toward_zero:
        over = np.abs(r.astype(np.float64)) > np.abs(x)
        r = np.where(over, np.nextafter(r, np.float16(0)), r)
    return r.astype(np.float64)


def rounder(tier, toward_zero=False):
    """x (float64 array) -> x rounded to the tier's operand type (f16: 10 mantissa bits; bf16: 7), as float64.  toward_zero: the
    WRONG rounding, for the model's own self-check."""
    fn = {"f16": _f16, "bf16": _bf16}[tier]
    return lambda x: fn(x, toward_zero)


def posenc16(p, n_freq):
    """the encoding as dfn_mlp.h posenc forms it in the 16-bit tiers: sin(2 pi (fract(p/2 * 2^(i-1)) + 1/4 [cos])) - power-of-two
    scalings and fract are exact in f32, the sine is evaluated exactly here (the hardware's is not: part of the gate's factor).
    p [N, 3] float32 -> [N, 6 n_freq] float64, columns as O.posenc."""
    ph = np.asarray(p, np.float32) * np.float32(0.5)
    out = []
    for i in range(n_freq):
        r = ph * np.float32(2.0 ** (i - 1))
        fr = (r - np.floor(r)).astype(np.float32)
        for q in (0.0, 0.25):
            out.append(np.sin(2.0 * np.pi * (fr + np.float32(q)).astype(np.float32).astype(np.float64)))
    return np.concatenate(out, -1)


class DenseReader:
    """test_pack_plan.Reader's interface on the dense weights of a state dict, for one field's program (head 0 / torso 1): the
    weight blocks in the kernels' consumption order, padded to the tile sizes - no packed stream, no library."""

    def __init__(self, field, state, flat):
        off, W = 0, {}
        for k, v in state.items():
            W[k] = np.asarray(flat[off:off + v.size], np.float64).reshape(v.shape)
            off += v.size
        assert off == len(flat)
        pad = lambda w, r, c: np.pad(w, ((0, r - w.shape[0]), (0, c - w.shape[1])))
        blk = lambda i: W[f"blocks.{i}.weight"]
        q = []
        if field == 0:
            q.append(pad(W["fc_in.weight"][:, :60], 256, 64))
            skip = pad(W["fc_p_skips.0.weight"][:, :60], 256, 64)
        else:
            d = lambda n: W[f"deform_net.{n}.weight"]
            q += [pad(d("blocks_embed.0")[:, :60], 64, 64), pad(d("blocks_signal.0")[:, :60], 64, 64)]
            q += [d("blocks_embed.1"), d("blocks_signal.1"), d("blocks_embed.2"), d("blocks_signal.2")]
            q += [(d("blocks_embed.3"), pad(d("fc_embed_skips.0"), 64, 64)), d("blocks_signal.3")]
            q += [d("blocks_embed.4"), d("blocks_signal.4"), pad(d("out_embed"), 64, 64), pad(d("out_signal"), 64, 64)]
            two = lambda w: np.concatenate([pad(w[:, :60], 256, 64), pad(w[:, 60:], 256, 64)], 1)
            q.append(two(W["fc_in_torso.weight"]))
            skip = two(W["fc_p_skips_torso.0.weight"])
        q += [blk(0), blk(1), blk(2), (blk(3), skip), blk(4), blk(5), blk(6)]
        fv, vw = W["feat_view.weight"], pad(W["fc_view.weight"], 256, 32)
        for tg in range(4):
            q += [fv[64 * tg:64 * tg + 64], vw[64 * tg:64 * tg + 64]]
        q += [pad(W["sigma_out.weight"], 32, 256), np.zeros((32, 32)), pad(W["feat_out.weight"], 32, 256)]
        self.queue, self.plan = q, None

    def _next(self, rows, cols):
        w = self.queue.pop(0)
        assert not isinstance(w, tuple) and w.shape == (rows, cols), (getattr(w, "shape", None), rows, cols)
        return w

    def group(self, G, KU, nslots):
        return self._next(32 * G, nslots)

    def layer(self, OT, KU, nslots):
        return self._next(32 * OT, nslots)

    def layer_skip(self, OT, KU, nslots, KU2, nslots2):
        a, b = self.queue.pop(0)
        assert a.shape == (32 * OT, nslots) and b.shape == (32 * OT, nslots2)
        return a, b


def model_fields(orc, z, tier, toward_zero=False):
    """the model decoder's (sigma_h, feat_h, sigma_t, feat_t) at depths z [n, S], float32 tensors: every GEMM operand of both
    fields rounded to `tier`'s type, everything else exact (float64)"""
    import test_pack_plan as tpp
    near = rounder(tier)
    rnd = near
    if toward_zero:                 # the WRONG model: activations truncated, weights and encodings rounded as they are
        trunc = rounder(tier, True)
        rnd = lambda x: trunc(x)
        rnd.weights = near
    z = t(np.asarray(z, np.float32))
    n, S = z.shape
    sg = [orc.sig[0][0].numpy().astype(np.float64), orc.sigt.reshape(-1).numpy().astype(np.float64)]
    out = []
    for f in (0, 1):
        o, d = orc.rays[2 * f], orc.rays[2 * f + 1]
        p = O.ray_points(o, d, z).reshape(-1, 3).numpy()                              # f32, as the kernel forms o + d z
        dh = (d / torch.norm(d, dim=-1, keepdim=True))[:, None, :].expand(n, S, 3).reshape(-1, 3).numpy()
        feat, sigma = tpp.emulate(1, f, orc.state, near(posenc16(p, 10)), near(posenc16(dh, 4)), sg[f],
                                  orc.zs[0, f].numpy().astype(np.float64), orc.za[0, f].numpy().astype(np.float64), rnd=rnd,
                                  reader=lambda flat, f=f: DenseReader(f, orc.state, flat))
        out += [t(sigma.reshape(n, S).astype(np.float32)), t(feat.reshape(n, S, 3).astype(np.float32))]
    return out


def image_errors(rgb, ref):
    """-> (rms over every entry, largest per-ray error = max over rays of the ray's largest channel error, PSNR in dB)"""
    d = np.asarray(rgb, np.float64) - np.asarray(ref, np.float64)
    mse = float((d * d).mean())
    return float(np.sqrt(mse)), float(np.abs(d).max(1).max()), (float("inf") if mse == 0 else -10.0 * np.log10(mse))
