"""The signal encoders' kernels (dfn_signal.hip: AudioNet_W2L, ExpressionEnc and the two AudioAttNets) per element against
float64: every backward entry point and the three forward ones over windows that overhang either end or both, every window
size the API accepts and both unsmoothed branches; what the accumulating and the overwriting variants leave in their buffers;
and the same gradients through training.SignalTrainer on all three dispatch paths of its backward.

The reference and the gate are tests/signal_ref.py (checked on the CPU by tests/test_signal_ref_host.py): per parameter
tensor |got - g64| <= 8 * max(e32, 2^-23 max|g64|), e32 = the float32 CPU autograd's own error against float64 in the same
case (and, inside a network, not below the median of e32 / max|g64| over its tensors: signal_ref.error_level has the one miss
of the first run that this answers).  Every launch is one workgroup (the batched forward: one per frame id) on a sequence
of at most eight frames."""
import ctypes as C

import numpy as np
import pytest
import torch

import signal_ref as R

pytestmark = pytest.mark.gpu

IDS = [R.case_id(c) for c in R.CASES]
AUDIO, TORSO = ("AudNet", "ExpNet", "AudAttNet"), ("PoseAttNet",)
AUDIO_ENTRIES = ("bwd", "bwd_set", "bwd_kept")
TORSO_ENTRIES = ("torso_bwd", "torso_bwd_set")


def t(x):
    return torch.from_numpy(np.asarray(x))


def p(x):
    return C.c_void_p(x.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Case:
    """device-side inputs of a case (never written)"""

    def __init__(self, states, scene, case):
        dev = torch.device("cuda")
        self.case = case
        self.N, self.frame, self.smo, self.smo_t = case
        self.st = R.case_states(states, case)
        self.par = {n: R.flat(self.st[n]).to(dev) for n in R.NETS}
        self.auds, self.exps = [t(scene[k])[:self.N].float().contiguous().to(dev) for k in ("aud", "exp")]
        poses = t(scene["poses"])[:self.N].float()
        self.poses = {16: poses.contiguous().to(dev), 12: poses[:, :3, :].contiguous().to(dev)}
        self.d, self.dt = [x.to(dev) for x in R.d_out()]
        self.ids = torch.tensor([self.frame], dtype=torch.int32, device=dev)

    def buffers(self, nets, fill=0.0):
        return {n: torch.full_like(self.par[n], fill) for n in nets}


_CASES = {}


def _case(states, scene, case):
    if case not in _CASES:
        _CASES[case] = _Case(states, scene, case)
    return _CASES[case]


def _keep_forward(c):
    from dfanerf._lib import check, lib
    keep = torch.zeros(check(lib.dfn_encode_signal_keep_floats(), "keep"), device="cuda")
    out = torch.empty(1, 96, device="cuda")
    check(lib.dfn_encode_signal_keep(p(c.par["AudNet"]), p(c.par["ExpNet"]), p(c.par["AudAttNet"]), p(c.auds), p(c.exps), c.N,
                                     p(c.ids), c.smo, p(out), p(keep), _st()), "encode_keep")
    return out, keep


def _run(c, entry, g, stride=16):
    """one backward entry point of the library on the buffers g {net: flat}"""
    from dfanerf._lib import check, lib
    if entry in AUDIO_ENTRIES:
        a = [p(c.par[n]) for n in AUDIO] + [p(c.auds), p(c.exps), c.N, c.frame, c.smo, p(c.d)]
        gs = [p(g[n]) for n in AUDIO]
        if entry == "bwd_kept":
            _, keep = _keep_forward(c)
            check(lib.dfn_encode_signal_bwd_kept(*a, p(keep), *gs, _st()), entry)
        else:
            check((lib.dfn_encode_signal_bwd_set if entry == "bwd_set" else lib.dfn_encode_signal_bwd)(*a, *gs, _st()), entry)
    else:
        fn = lib.dfn_encode_signal_torso_bwd_set if entry == "torso_bwd_set" else lib.dfn_encode_signal_torso_bwd
        check(fn(p(c.par["PoseAttNet"]), p(c.poses[stride]), stride, c.N, c.frame, c.smo_t, p(c.dt), p(g["PoseAttNet"]), _st()), entry)
    torch.cuda.synchronize()
    return g


def _nets(entry):
    return AUDIO if entry in AUDIO_ENTRIES else TORSO


def _part(c, n):
    """does network n take part in the case?"""
    return {"AudNet": True, "ExpNet": True, "AudAttNet": c.smo > 0, "PoseAttNet": c.smo_t > 0}[n]


def _bits(x):
    return x.view(torch.int32)


_ZERO = {}


def _from_zero(c, entry):
    """what an entry point leaves in zero-filled buffers (computed once per case and entry point, not modified)"""
    key = (c.case, entry)
    if key not in _ZERO:
        _ZERO[key] = _run(c, entry, c.buffers(_nets(entry)))
    return _ZERO[key]


# ---- (a) forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_forward_vs_float64(states, scene, case):
    """dfn_encode_signal and dfn_encode_signal_torso (both pose strides) on an id list with both edge frames and a repeated id -
    those of them at which the reference's zero padding is defined: in the three-frame sequence frame 0 would need four padded
    rows from three - and dfn_encode_signal_keep at the case's frame: the 96 and 42 outputs under the gradients' gate."""
    from dfanerf._lib import check, lib
    c = _case(states, scene, case)
    dev = torch.device("cuda")
    worst = 0.0
    want = [c.frame, 0, c.N - 1, c.frame]
    for side, smo in (("audio", c.smo), ("torso", c.smo_t)):
        ids = [i for i in want if R.in_domain(c.N, i, smo)]
        assert len(ids) >= 3 and len(set(ids)) < len(ids) and (c.N == 3 or {0, c.N - 1} <= set(ids))
        ids_d = torch.tensor(ids, dtype=torch.int32, device=dev)
        k = 0 if side == "audio" else 1
        refs = [(R.forward_sides(states, scene, case, i)[k], R.forward_sides(states, scene, case, i, torch.float32)[k]) for i in ids]
        outs = []
        if side == "audio":
            out = torch.full((len(ids), 96), float("nan"), device=dev)
            check(lib.dfn_encode_signal(p(c.par["AudNet"]), p(c.par["ExpNet"]), p(c.par["AudAttNet"]), p(c.auds), p(c.exps), c.N,
                                        p(ids_d), len(ids), smo, p(out), _st()), "encode")
            outs.append(("dfn_encode_signal", out))
            one, _ = _keep_forward(c)
            torch.cuda.synchronize()
            assert torch.equal(one[0], out[0])
            err, tol, ok = R.gate_tensor(one[0], *refs[0])
            assert ok, ("dfn_encode_signal_keep", err, tol)
        else:
            for stride in (16, 12):
                out = torch.full((len(ids), 42), float("nan"), device=dev)
                check(lib.dfn_encode_signal_torso(p(c.par["PoseAttNet"]), p(c.poses[stride]), stride, c.N, p(ids_d), len(ids), smo,
                                                  p(out), _st()), "encode_torso")
                outs.append((f"dfn_encode_signal_torso stride {stride}", out))
        torch.cuda.synchronize()
        for name, out in outs:
            assert torch.equal(out[0], out[-1])                    # the repeated id
            for row, i, (r64, r32) in zip(out, ids, refs):
                err, tol, ok = R.gate_tensor(row, r64, r32)
                assert ok, (name, i, err, tol)
                worst = max(worst, err / tol)
    print(f"signal forward {R.case_id(case)}: worst error / tolerance {worst:.3f}")


# ---- (b) backward, every entry point, every element -----------------------------------------------------------------------
@pytest.mark.parametrize("entry", AUDIO_ENTRIES + TORSO_ENTRIES)
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_backward_vs_float64(states, scene, case, entry):
    c = _case(states, scene, case)
    g = _from_zero(c, entry)
    got = {n: (g[n] if _part(c, n) else None) for n in _nets(entry)}
    own = []
    bad, worst = R.gate_case(got, states, scene, case, nets=_nets(entry), plain=own)
    print(f"signal backward dfn_encode_signal_{entry} {R.case_id(case)}: worst error / tolerance {worst:.3f} (each tensor on its own: {own[0]:.3f})")
    assert not bad, bad
    for n in _nets(entry):                                         # a network that takes no part: not written
        assert _part(c, n) or not bool(g[n].any())
    if entry == "torso_bwd" and c.smo_t:                            # the other pose stride: the same bits
        g12 = _run(c, entry, c.buffers(TORSO), stride=12)
        assert torch.equal(g12["PoseAttNet"], g["PoseAttNet"])


# ---- (c) buffer semantics ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ("bwd", "bwd_kept", "torso_bwd"))
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_accumulating_variants_add_onto_the_buffer(states, scene, case, entry):
    """Started on a seeded non-zero buffer b (per tensor a quarter of that tensor's largest gradient entry, times randn) they
    leave b + g.  The error against the float64 b + g64 - which is the error of (result - b) against g64 - under the gradient's
    own gate: the buffer adds half an ulp of |b + g| <= 2^-24 * 2.2 max|g64| to the float32 sum, inside the gate's 8 * 2^-23
    max|g64| floor.  (Sizing e32 from the float32 sum b + g32 instead would let b decide the tolerance where b + g cancels:
    measured on the first run, the one-entry attentionConvNet.8.bias of (3, 1, 8, 8) then has 2.8e-7 for the kernel's 2.1e-6.)"""
    c = _case(states, scene, case)
    r64 = R.reference(states, scene, case)[0].grads
    gen = torch.Generator().manual_seed(7)
    b = {}
    for n in _nets(entry):
        b[n] = torch.randn(c.par[n].numel(), generator=gen)
        if r64[n] is not None:
            for _, o, k in R.slices(c.st[n]):
                b[n][o:o + k] *= 0.25 * float(r64[n][o:o + k].abs().max())
        assert bool((b[n] != 0).all())
    g = _run(c, entry, {n: v.to("cuda") for n, v in b.items()})
    got = {n: (g[n].cpu().double() - b[n].double() if _part(c, n) else None) for n in _nets(entry)}
    own = []
    bad, worst = R.gate_case(got, states, scene, case, nets=_nets(entry), plain=own)
    print(f"signal backward onto a buffer dfn_encode_signal_{entry} {R.case_id(case)}: worst error / tolerance {worst:.3f} (each tensor on its own: {own[0]:.3f})")
    assert not bad, bad
    for n in _nets(entry):
        assert _part(c, n) or torch.equal(g[n].cpu(), b[n])         # no part: untouched


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_set_variants_overwrite_and_idle_buffers_stay(states, scene, case):
    """The _set variants on NaN-filled buffers: finite, and bit for bit the accumulating variant from zero - the audio pair and
    the torso pair.  An unsmoothed branch: the attention buffer keeps its NaN fill under all three audio variants, and the
    torso calls write nothing."""
    c = _case(states, scene, case)
    nan = float("nan")
    for acc, st_ in (("bwd", "bwd_set"), ("torso_bwd", "torso_bwd_set")):
        ref = _from_zero(c, acc)
        g = _run(c, st_, c.buffers(_nets(st_), nan))
        for n in _nets(st_):
            if _part(c, n):
                assert bool(torch.isfinite(g[n]).all()) and torch.equal(g[n], ref[n]), (st_, n)
            else:
                assert bool(torch.isnan(g[n]).all()), (st_, n)
    idle = [n for n in R.NETS if not _part(c, n)]
    for entry in AUDIO_ENTRIES + TORSO_ENTRIES:
        if not set(idle) & set(_nets(entry)):
            continue
        g = c.buffers(_nets(entry))
        for n in idle:
            if n in g:
                g[n].fill_(nan)
        g = _run(c, entry, g)
        for n in _nets(entry):
            if n in idle:
                assert bool(torch.isnan(g[n]).all()), (entry, n)
            else:
                assert torch.equal(g[n], _from_zero(c, "bwd")[n]), (entry, n)


# ---- (d) the three audio variants, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_three_audio_variants_are_bit_equal(states, scene, case):
    from dfanerf._lib import check, lib
    c = _case(states, scene, case)
    plain = torch.empty(1, 96, device="cuda")
    check(lib.dfn_encode_signal(p(c.par["AudNet"]), p(c.par["ExpNet"]), p(c.par["AudAttNet"]), p(c.auds), p(c.exps), c.N, p(c.ids), 1,
                                c.smo, p(plain), _st()), "encode")
    kept, _ = _keep_forward(c)
    torch.cuda.synchronize()
    assert torch.equal(_bits(plain), _bits(kept))
    g0, g1 = _from_zero(c, "bwd"), _from_zero(c, "bwd_kept")
    g2 = _run(c, "bwd_set", c.buffers(AUDIO, 7.0))
    for n in AUDIO:
        assert torch.equal(_bits(g0[n]), _bits(g1[n])), n
        if _part(c, n):
            assert torch.equal(_bits(g0[n]), _bits(g2[n])) and float(g0[n].abs().max()) > 0, n
        else:
            assert bool((g2[n] == 7.0).all()), n


# ---- (e) through training.SignalTrainer ---------------------------------------------------------------------------------
MODES = {"kept": (False, True), "set": (True, True), "recompute": (False, False)}      # (_SIG_SET, _SIG_KEEP)


def _trainer(states, scene, case, monkeypatch, mode="kept"):
    """fresh modules and a trainer for a case, the backward's dispatch pinned to a mode"""
    from dfanerf import nets, training
    monkeypatch.setattr(training, "_SIG_SET", MODES[mode][0])
    monkeypatch.setattr(training, "_SIG_KEEP", MODES[mode][1])
    N, _, smo, smo_t = case
    st = R.case_states(states, case)
    mods = {"AudNet": nets.AudioNet_W2L(), "ExpNet": nets.ExpressionEnc(), "AudAttNet": nets.AudioAttNet(96, smo or 4),
            "PoseAttNet": nets.AudioAttNet(42, smo_t or 8)}
    for k, m in mods.items():
        m.load_state_dict({kk: t(v) for kk, v in st[k].items()})
        m.cuda()
    auds, exps, poses = [t(scene[k])[:N].float().cuda() for k in ("aud", "exp", "poses")]
    return mods, training.SignalTrainer(mods["AudNet"], mods["ExpNet"], mods["AudAttNet"], mods["PoseAttNet"], auds, exps, poses)


def _step(tr, case):
    """encode a case and the scalar whose backward sends the seeded d_sig / d_sigt into the encoders"""
    N, frame, smo, smo_t = case
    sig, sigt = tr.encode(frame, smo, smo_t, N)
    d, dt = [x.cuda() for x in R.d_out()]
    return sig, sigt, (sig.reshape(-1) * d).sum() + (sigt.reshape(-1) * dt).sum()


def _module_grads(tr, mods):
    tr.join()
    torch.cuda.synchronize()
    out = {}
    for n, m in mods.items():
        gs = [q.grad for q in m.state_dict(keep_vars=True).values()]
        assert all(g is None for g in gs) or all(g is not None for g in gs), n
        out[n] = None if gs[0] is None else torch.cat([g.reshape(-1) for g in gs]).cpu()
    return out


def _sum(a, b):
    return {n: None if a[n] is None else a[n] + b[n] for n in R.NETS}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_trainer_gradients_vs_float64(states, scene, case, mode, monkeypatch):
    """encode() and backward leave .grad on the four modules within the gate (the signals too), on each dispatch path of
    _SignalFn.backward; an attention module of an unsmoothed branch keeps .grad None"""
    mods, tr = _trainer(states, scene, case, monkeypatch, mode)
    sig, sigt, loss = _step(tr, case)
    loss.backward()
    got = _module_grads(tr, mods)
    r64, r32 = R.reference(states, scene, case)
    for out, a, b in ((sig, r64.sig, r32.sig), (sigt, r64.sigt, r32.sigt)):
        err, tol, ok = R.gate_tensor(out.detach().reshape(-1), a, b)
        assert ok, (err, tol)
    own = []
    bad, worst = R.gate_case(got, states, scene, case, plain=own)
    print(f"SignalTrainer {mode} {R.case_id(case)}: worst error / tolerance {worst:.3f} (each tensor on its own: {own[0]:.3f})")
    assert not bad, bad
    if case[2] == 0:
        assert all(q.grad is None for q in mods["AudAttNet"].parameters())
    if case[3] == 0:
        assert all(q.grad is None for q in mods["PoseAttNet"].parameters())


PAIRS = [((8, 3, 4, 8), (8, 6, 4, 8)), ((8, 0, 8, 8), (8, 7, 8, 8))]


@pytest.mark.parametrize("pair", PAIRS, ids=["interior", "both-ends"])
def test_trainer_second_backward_accumulates(states, scene, pair, monkeypatch):
    """a second forward and backward at another frame without zeroing: .grad holds the sum of the two float64 gradients
    (_FlatNet.deposit adds onto an existing .grad)"""
    A, B = pair
    mods, tr = _trainer(states, scene, A, monkeypatch)
    for case in (A, B):
        _step(tr, case)[2].backward()
    got = _module_grads(tr, mods)
    (a64, a32), (b64, b32) = R.reference(states, scene, A), R.reference(states, scene, B)
    own = []
    bad, worst = R.gate_case(got, states, scene, A, r64=_sum(a64.grads, b64.grads), r32=_sum(a32.grads, b32.grads), plain=own)
    print(f"SignalTrainer two backwards {R.case_id(A)} + {R.case_id(B)}: worst error / tolerance {worst:.3f} (each tensor on its own: {own[0]:.3f})")
    assert not bad, bad
    # ... and the sum is not either gradient alone, by far more than the gate
    for one in (a64, b64):
        assert R.gate_case(one.grads, states, scene, A, r64=_sum(a64.grads, b64.grads), r32=_sum(a32.grads, b32.grads))[1] >= 100.0


def test_trainer_backward_of_an_earlier_encode_recomputes(states, scene, monkeypatch):
    """encode(A), encode(B), backward of A's outputs alone: A's gradient - the kept activations are B's by then, and
    _SignalFn.backward must not use them (ctx.keep_seq).  B's backward afterwards (the latest encode: the kept path) adds B's."""
    A, B = PAIRS[0]
    mods, tr = _trainer(states, scene, A, monkeypatch, "kept")
    (a64, a32), (b64, b32) = R.reference(states, scene, A), R.reference(states, scene, B)
    assert R.gate_case(b64.grads, states, scene, A)[1] >= 100.0        # the two frames' gradients differ by far more than the gate
    loss_a = _step(tr, A)[2]
    loss_b = _step(tr, B)[2]
    loss_a.backward()
    own = []
    bad, worst = R.gate_case(_module_grads(tr, mods), states, scene, A, plain=own)
    print(f"SignalTrainer stale keep {R.case_id(A)}: worst error / tolerance {worst:.3f} (each tensor on its own: {own[0]:.3f})")
    assert not bad, bad
    loss_b.backward()
    bad, _ = R.gate_case(_module_grads(tr, mods), states, scene, A, r64=_sum(a64.grads, b64.grads), r32=_sum(a32.grads, b32.grads))
    assert not bad, bad
