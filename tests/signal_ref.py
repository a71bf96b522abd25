"""Float64 reference of the two signal encoders (rows A7 / A8) and of their parameter gradients, the per-element gate the
GPU tests hold the HIP backward kernels to, and the deliberately wrong references that show what the gate can see.  No GPU.

The reference is autograd through oracle/dfa_oracle.py's encode_signal / encode_signal_torso with .double() parameters and
inputs; the same computation in float32 only sizes the tolerance.  Gradients come back as one flat vector per network in
state_dict order - the layout of the kernels' gradient buffers.

The gate, per parameter tensor:  |got - g64| <= 8 * max(e32, 2^-23 * max|g64|)  for every entry, where e32 is the largest
error over that tensor of the float32 CPU gradient against the float64 one, computed for the same case.  Why 8: the kernels
sum dot products of up to 512 terms as one sequential fmaf chain where torch sums in blocks of eight or more; for rounding
errors of random sign that costs about sqrt(512 / 8) = 8 in the worst layer and nothing in the attention stack.  A tensor
whose float64 gradient is exactly zero must be exactly zero.  One refinement, from the first run on the device (error_level
has the finding and the figures): inside a network's gradient a tensor's e32 is not taken below the median of e32 / max|g64|
over that network's tensors, times its own max|g64| - a tensor of one or two entries draws the float32 error once or twice
and can land twenty times under the level all its neighbours show."""
import numpy as np
import torch
import torch.nn.functional as F

import dfa_oracle as O
from dfanerf import synth

NOSMO = 300000
NETS = ("AudNet", "ExpNet", "AudAttNet", "PoseAttNet")
# (N, frame, smo, smo_t): the sequence is the first N frames of the session scene
CASES = [
    (8, 3, 4, 8),        # the suite's existing case
    (8, 0, 8, 8),        # left overhang
    (8, 7, 8, 8),        # right overhang
    (3, 1, 8, 8),        # overhang on both sides
    (8, 0, 2, 2),        # smallest window, left end
    (8, 7, 6, 6),        # right end
    (8, 4, 6, 2),        # interior, different windows
    (8, 2, 0, 0),        # unsmoothed branch
    (8, 5, 0, 8),        # mixed branches
    (8, 5, 4, 0),        # mixed branches
]
MUTANTS = ("shift", "drop_last", "leaky_pad", "no_direct", "no_dot", "bias_cut")
GATE_FACTOR = 8.0


def case_id(case):
    return "N%d-f%d-smo%d-smot%d" % tuple(case)


def t(x):
    return torch.from_numpy(np.asarray(x))


def att_state(dim, seq_len, seed=0):
    """Seeded parameters of nets.AudioAttNet(dim, seq_len) for any window size (dim 96: the audio net, 42: the pose net).  The
    values are synth's hash of (seed, tensor name, index): with seed 0 the nets of the suite's own states (AudioAttNet(96, 4),
    AudioAttNet(42, 8)) come out unchanged, and the conv stack is the same at every window size."""
    assert dim in (96, 42) and seq_len in (2, 4, 6, 8)
    return synth.synth_state(synth.attnet_shapes(dim, seq_len), seed, "AudAttNet" if dim == 96 else "PoseAttNet")


def case_states(states, case):
    """The four networks' parameters (numpy, state_dict order) for a case: the session's AudNet / ExpNet and attention nets of
    the case's window sizes (the session's own where a branch is unsmoothed: that net then takes no part)."""
    _, _, smo, smo_t = case
    return {"AudNet": states["AudNet"], "ExpNet": states["ExpNet"],
            "AudAttNet": att_state(96, smo) if smo else states["AudAttNet"],
            "PoseAttNet": att_state(42, smo_t) if smo_t else states["PoseAttNet"]}


def flat(state):
    """one network's tensors as the kernels see them: a flat f32 vector in state_dict order"""
    return torch.cat([t(v).reshape(-1) for v in state.values()]).float().contiguous()


def slices(state):
    """[(tensor name, offset, count)] of a network's flat vector"""
    out, o = [], 0
    for k, v in state.items():
        n = int(np.prod(np.shape(v)))
        out.append((k, o, n))
        o += n
    return out


def window_pads(frame, smo, N):
    """(pad_l, rows, pad_r) of the window [frame - smo/2, frame + smo/2) clipped to [0, N)"""
    half = smo // 2
    left, right = frame - half, frame + half
    pad_l, pad_r = max(0, -left), max(0, right - N)
    return pad_l, min(right, N) - max(left, 0), pad_r


def in_domain(N, frame, smo):
    """The oracle pads with zeros_like(win)[:pad]: at most as many rows as the clipped window holds."""
    if smo == 0:
        return 0 <= frame < N
    pad_l, rows, pad_r = window_pads(frame, smo, N)
    return rows > 0 and pad_l <= rows and pad_r <= rows


def d_out():
    """the seeded gradients that enter the encoders: d_sig [96], d_sigt [42] (float32 values)"""
    g = torch.Generator().manual_seed(20240607)
    return torch.randn(96, generator=g), torch.randn(42, generator=g)


# ---- the encoders restated with switches (only the mutants use the switches; without one this is the oracle) ----------
class _SoftmaxNoDot(torch.autograd.Function):
    """softmax whose backward forgets the - sum_j att[j] d_att[j] term"""

    @staticmethod
    def forward(ctx, z):
        a = F.softmax(z, dim=1)
        ctx.save_for_backward(a)
        return a

    @staticmethod
    def backward(ctx, d):
        return ctx.saved_tensors[0] * d


def _cut_bias(b, axis_len):
    """bias broadcast over `axis_len` window rows whose gradient sums over the first axis_len - 1 rows only (same values)"""
    m = torch.ones(axis_len, dtype=b.dtype)
    m[-1] = 0
    return b[None, :] * m[:, None] + b.detach()[None, :] * (1 - m)[:, None]


def _lin(P, name, x, mutant):
    if mutant == "bias_cut":
        return F.linear(x, P[name + ".weight"]) + _cut_bias(P[name + ".bias"], x.shape[0])
    return F.linear(x, P[name + ".weight"], P[name + ".bias"])


def _act(x, pad_rows, mutant):
    y = F.leaky_relu(x, 0.02)
    if mutant == "leaky_pad":
        y = torch.where(pad_rows[:, None], x, y)       # slope 1 on the zero-padded rows
    return y


def _att(P, x, dim, S, mutant):
    y = x[..., :dim].permute(1, 0).unsqueeze(0)
    for k in range(5):
        W, b = P[f"attentionConvNet.{2 * k}.weight"], P[f"attentionConvNet.{2 * k}.bias"]
        if mutant == "bias_cut":
            y = F.conv1d(y, W, None, padding=1) + _cut_bias(b, S).permute(1, 0).unsqueeze(0)
        else:
            y = F.conv1d(y, W, b, padding=1)
        y = F.leaky_relu(y, 0.02)
    z = _lin(P, "attentionNet.0", y.view(1, S), None)
    a = (_SoftmaxNoDot.apply(z) if mutant == "no_dot" else F.softmax(z, dim=1)).view(S, 1)
    return torch.sum(a * (x.detach() if mutant == "no_direct" else x), dim=0)


def _win(x, frame, smo, N, mutant):
    """(window rows [S, D] with zero padding, bool [S] marking the padded rows)"""
    if smo == 0:
        w, pad = x[frame:frame + 1], torch.zeros(1, dtype=torch.bool)
    else:
        pad_l, rows, pad_r = window_pads(frame, smo, N)
        lo = max(frame - smo // 2, 0)
        z = x.new_zeros
        w = torch.cat((z(pad_l, x.shape[1]), x[lo:lo + rows], z(pad_r, x.shape[1])), 0)
        pad = torch.tensor([True] * pad_l + [False] * rows + [True] * pad_r)
    if mutant == "drop_last":
        w = torch.cat((w[:-1], torch.zeros_like(w[-1:])), 0)
    return w, pad


def encode_switched(P, auds, exps, poses, case, mutant=None):
    """sig [96], sigt [42] of a case; mutant = None or one of MUTANTS"""
    N, frame, smo, smo_t = case
    if mutant == "shift":
        frame = frame + 1 if frame + 1 < N else frame - 1
    xa, pad = _win(auds, frame, smo, N, mutant)
    xe, _ = _win(exps, frame, smo, N, mutant)
    A, E = P["AudNet"], P["ExpNet"]
    h = _act(_lin(A, "encoder.0", xa, mutant), pad, mutant)
    h = _act(_lin(A, "encoder.2", h, mutant), pad, mutant)
    a = _lin(A, "encoder.4", h, mutant)
    e = _lin(E, "encoder.2", _act(_lin(E, "encoder.0", xe, mutant), pad, mutant), mutant)
    feat = torch.cat([a, e], 1)
    sig = _att(P["AudAttNet"], feat, 96, smo, mutant) if smo else feat.reshape(-1)
    et, _ = _win(O.pose_to_euler_trans(poses), frame, smo_t, N, mutant)
    emb = torch.cat((O.embed3(et[:, :3]), O.embed3(et[:, 3:])), 1)
    sigt = _att(P["PoseAttNet"], emb, 42, smo_t, mutant) if smo_t else emb.reshape(-1)
    return sig, sigt


def encode_oracle(P, auds, exps, poses, case):
    N, frame, smo, smo_t = case
    assert in_domain(N, frame, smo) and in_domain(N, frame, smo_t), f"{case}: outside the reference's domain"
    sig = O.encode_signal(P, auds, exps, frame, NOSMO if smo else 0, NOSMO, smo, N)[0].reshape(-1)
    sigt = O.encode_signal_torso(P, poses, frame, NOSMO if smo_t else 0, NOSMO, smo_t, N).reshape(-1)
    return sig, sigt


def forward_sides(states, scene, case, frame, dtype=torch.float64):
    """(sig [96] or None, sigt [42] or None) of the oracle at `frame` of the case's sequence, networks and windows, without
    gradients (the batched forward's other frames).  None: that side's window is outside the reference's domain there."""
    N, _, smo, smo_t = case
    st = case_states(states, case)
    P = {n: {k: t(v).to(dtype) for k, v in st[n].items()} for n in NETS}
    auds, exps, poses = [t(scene[k])[:N].to(dtype) for k in ("aud", "exp", "poses")]
    with torch.no_grad():
        sig = O.encode_signal(P, auds, exps, frame, NOSMO if smo else 0, NOSMO, smo, N)[0].reshape(-1) \
            if in_domain(N, frame, smo) else None
        sigt = O.encode_signal_torso(P, poses, frame, NOSMO if smo_t else 0, NOSMO, smo_t, N).reshape(-1) \
            if in_domain(N, frame, smo_t) else None
    return sig, sigt


class Ref:
    """outputs and gradients of one case in one precision: sig [96], sigt [42], grads {net: flat vector or None}
    (None: the network takes no part - an attention net of an unsmoothed branch)"""

    def __init__(self, sig, sigt, grads):
        self.sig, self.sigt, self.grads = sig, sigt, grads


def compute(states, scene, case, dtype=torch.float64, mutant=None, oracle=True):
    """Forward and autograd of loss = sig . d_sig + sigt . d_sigt for a case.  oracle: through dfa_oracle (the reference);
    otherwise through encode_switched (the mutants, and its own check against the oracle)."""
    N = case[0]
    st = case_states(states, case)
    P = {n: {k: t(v).to(dtype).clone().requires_grad_(True) for k, v in st[n].items()} for n in NETS}
    auds, exps, poses = [t(scene[k])[:N].to(dtype) for k in ("aud", "exp", "poses")]
    if oracle:
        assert mutant is None
        sig, sigt = encode_oracle(P, auds, exps, poses, case)
    else:
        sig, sigt = encode_switched(P, auds, exps, poses, case, mutant)
    d, dt = [x.to(dtype) for x in d_out()]
    loss = (sig * d).sum() + (sigt * dt).sum()
    leaves = [p for n in NETS for p in P[n].values()]
    got = iter(torch.autograd.grad(loss, leaves, allow_unused=True))
    grads = {}
    for n in NETS:
        gs = [next(got) for _ in P[n]]
        if all(g is None for g in gs):
            grads[n] = None
        else:
            grads[n] = torch.cat([(torch.zeros_like(p) if g is None else g).reshape(-1) for g, p in zip(gs, P[n].values())])
    return Ref(sig.detach(), sigt.detach(), grads)


_CACHE = {}


def reference(states, scene, case):
    """(float64 Ref, float32 Ref) of a case through the oracle, computed once per process and never modified"""
    key = tuple(case)
    if key not in _CACHE:
        _CACHE[key] = (compute(states, scene, case, torch.float64), compute(states, scene, case, torch.float32))
    return _CACHE[key]


# ---- the gate ---------------------------------------------------------------------------------------------------------
def tolerance(g64, g32, level=0.0):
    """8 * max(e32, level * max|g64|, 2^-23 max|g64|); level: the network's error level (gate), 0 for a tensor on its own"""
    m = float(g64.abs().max())
    return GATE_FACTOR * max(float((g32.double() - g64).abs().max()), level * m, 2.0 ** -23 * m)


def gate_tensor(got, g64, g32, level=0.0):
    """(error, tolerance, passed) of one tensor.  got: what is tested (any float dtype), g64 / g32: the float64 reference and
    the float32 CPU computation of the same thing."""
    got = got.detach().cpu().double().reshape(-1)
    g64 = g64.reshape(-1)
    tol = tolerance(g64, g32.reshape(-1), level)
    err = float((got - g64).abs().max())
    if float(g64.abs().max()) == 0.0:
        return err, 0.0, bool((got == 0).all())
    return err, tol, bool(err <= tol)          # (NaN: not passed)


def error_level(r64, r32, sl):
    """The float32 reference's error level of one network: the MEDIAN over its parameter tensors of e32 / max|g64|.

    Why the gate needs it.  e32 of a tensor is the largest of as many draws of the float32 rounding error as the tensor has
    entries, and attentionConvNet.8.bias has one.  First run on the MI355X, case (3, 1, 8, 8), all three audio entry points:
    that entry 2.06e-6 off float64 at a value of 0.966 - error / tolerance 2.24 under the plain rule, the one miss in 143 tests
    (everything else <= 0.45).  The kernel is not worse there: all gradients of an attention net are linear images of the same
    back-propagated vector dz[S] = att * (d_att - dot) (here d_att down to -10.9, dot -3.74, from feature rows that carry the
    512-term chains' rounding), so they share one relative error, and the float32 CPU autograd shows it on the eleven other
    tensors of that net: e32 = 0.9e-6 ... 2.8e-6 of the tensor's largest entry.  On the one-entry tensor its single draw on
    that host's CPU was <= 1.2e-7 (the 2^-23 floor decided); the same draw on the build host's CPU is 2.3e-6.  The kernel's
    2.1e-6 is the level, the reference's draw was the outlier.  So a tensor's e32 is not allowed to fall below the level its
    network's tensors show, taken as the median so that neither a lucky nor an unlucky draw moves it.  This comes from the
    reference alone, widens nothing above the median, and every mutant of test_signal_ref_host.py still fails by a factor
    >= 100.  With it the worst tensor of that case sits at error / tolerance 0.26 (measured, MI355X host)."""
    lv = []
    for _, o, n in sl:
        m = float(r64[o:o + n].abs().max())
        if m > 0:
            lv.append(float((r32[o:o + n].double() - r64[o:o + n]).abs().max()) / m)
    return float(np.median(lv)) if lv else 0.0


def gate(got, r64, r32, sl):
    """Per parameter tensor of one network: [(name, error, tolerance, passed, tolerance of the tensor on its own)].
    got / r64 / r32: flat vectors."""
    level = error_level(r64, r32, sl)
    return [(k,) + gate_tensor(got[o:o + n], r64[o:o + n], r32[o:o + n], level) + (tolerance(r64[o:o + n], r32[o:o + n]),)
            for k, o, n in sl]


def gate_case(got, states, scene, case, r64=None, r32=None, nets=NETS, plain=None):
    """Gate the gradients {net: flat vector or None} of a whole case against its reference.  Returns (failures, worst error /
    tolerance): failures = ["net/tensor: error > tolerance"].  A network the reference gives no gradient (None) must come
    without one (None).  nets: the networks an entry point writes.  plain: a list that receives the worst error / tolerance
    with every tensor's tolerance taken on its own (reported next to the gate's; error_level says why it does not gate)."""
    if r64 is None:
        r64, r32 = [r.grads for r in reference(states, scene, case)]
    st = case_states(states, case)
    bad, worst, worst_plain = [], 0.0, 0.0
    for n in nets:
        if r64[n] is None:
            if got.get(n) is not None:
                bad.append(f"{n}: a gradient where the reference has none")
            continue
        if got.get(n) is None:
            bad.append(f"{n}: no gradient")
            continue
        for k, err, tol, ok, tol_own in gate(got[n], r64[n], r32[n], slices(st[n])):
            if tol > 0:
                worst = max(worst, err / tol) if err == err else float("inf")
                worst_plain = max(worst_plain, err / tol_own) if err == err else float("inf")
            if not ok:
                bad.append(f"{n}/{k}: {err:.3e} > {tol:.3e}")
    if plain is not None:
        plain.append(worst_plain)
    return bad, worst


def mutant_applies(mutant, case):
    """does the mutation change any gradient of this case?"""
    N, frame, smo, smo_t = case
    pa, pt = window_pads(frame, smo, N) if smo else (0, 1, 0), window_pads(frame, smo_t, N) if smo_t else (0, 1, 0)
    if mutant in ("shift", "bias_cut"):
        return True
    if mutant == "drop_last":                     # the last row holds data on the audio side, or on a smoothed pose side
        return pa[2] == 0 or (smo_t > 0 and pt[2] == 0)
    if mutant == "leaky_pad":                     # the AudNet / ExpNet layers see a padded row
        return smo > 0 and (pa[0] > 0 or pa[2] > 0)
    if mutant == "no_direct":                     # parameters in front of an attention net: the audio side only
        return smo > 0
    if mutant == "no_dot":
        return smo > 0 or smo_t > 0
    raise ValueError(mutant)
