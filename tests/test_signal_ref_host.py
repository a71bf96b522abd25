"""tests/signal_ref.py on the CPU: the float64 reference of the signal encoders is the oracle and the torch twins, the gate
accepts the float32 CPU gradients of every case, and it rejects every deliberately wrong reference - the errors a kernel of
the shape of dfn_signal.hip's backward can make - without rebuilding any kernel."""
import numpy as np
import pytest
import torch

import signal_ref as R
from dfanerf import nets

IDS = [R.case_id(c) for c in R.CASES]


def t(x):
    return torch.from_numpy(np.asarray(x))


def test_case_matrix_is_inside_the_references_domain():
    assert len(R.CASES) == 10 and len(set(R.CASES)) == 10
    for N, frame, smo, smo_t in R.CASES:
        assert R.in_domain(N, frame, smo) and R.in_domain(N, frame, smo_t)
    assert not R.in_domain(1, 0, 8)               # (N = 1, smo = 8): the reference cannot pad four rows from one
    assert R.window_pads(1, 8, 3) == (3, 3, 2)
    assert R.window_pads(0, 2, 8) == (1, 1, 0) and R.window_pads(7, 6, 8) == (0, 4, 2)


def test_attention_builder_matches_the_modules_and_the_session_states(states):
    for dim in (96, 42):
        for S in (2, 4, 6, 8):
            st = R.att_state(dim, S)
            mod = nets.AudioAttNet(dim, S)
            assert list(st.keys()) == list(mod.state_dict().keys())
            mod.load_state_dict({k: t(v) for k, v in st.items()})            # shapes
            assert R.flat(st).numel() == sum(p.numel() for p in mod.parameters())
            other = R.att_state(dim, S, seed=1)
            assert not np.array_equal(other["attentionNet.0.weight"], st["attentionNet.0.weight"])
    for name, dim, S in (("AudAttNet", 96, 4), ("PoseAttNet", 42, 8)):
        st = R.att_state(dim, S)
        assert all(np.array_equal(st[k], states[name][k]) for k in states[name])


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_float32_forward_is_the_torch_twins(states, scene, case):
    N, frame, smo, smo_t = case
    st = R.case_states(states, case)
    mods = {"AudNet": nets.AudioNet_W2L(), "ExpNet": nets.ExpressionEnc(), "AudAttNet": nets.AudioAttNet(96, smo or 4),
            "PoseAttNet": nets.AudioAttNet(42, smo_t or 8)}
    for k, m in mods.items():
        m.load_state_dict({kk: t(v) for kk, v in st[k].items()})
    ds = [{"auds": t(scene["aud"])[:N], "exp": t(scene["exp"])[:N], "poses": t(scene["poses"])[:N]}]
    embed_fn, _ = nets.get_embedder(3, 0)

    class A:
        nosmo_iters, smo_size, smo_torse_size = R.NOSMO, smo, smo_t
    with torch.no_grad():
        sig = nets.encode_signal(ds, 0, frame, 96, mods["AudNet"], mods["ExpNet"], mods["AudAttNet"], R.NOSMO if smo else 0, A, N)[0]
        sigt = nets.encode_signal_torso(ds, 0, frame, mods["PoseAttNet"], R.NOSMO if smo_t else 0, A, N, embed_fn=embed_fn)
    r32 = R.reference(states, scene, case)[1]
    assert r32.sig.dtype == torch.float32 and r32.sig.shape == (96,) and r32.sigt.shape == (42,)
    assert torch.equal(r32.sig, sig.reshape(-1)) and torch.equal(r32.sigt, sigt.reshape(-1))


def test_float64_forward_reproduces_golden_g6(golden, states, scene):
    """every entry of G6 (window 4 / 8 and the unsmoothed branch at frames 0, 1, 4, 7 of the eight; frame 5 of a sequence cut to
    six), the matrix's own (8, 0, 8, 8) and (8, 7, 8, 8) pose sides among them"""
    g = golden("g6_signals")
    close = lambda a, b: np.testing.assert_allclose(a.numpy(), b.reshape(-1), rtol=1e-5, atol=1e-6)
    for i in (0, 1, 4, 7):
        for tag, smo, smo_t in (("raw", 0, 0), ("smo", 4, 8)):
            r = R.compute(states, scene, (8, i, smo, smo_t))
            assert r.sig.dtype == torch.float64
            close(r.sig, g[f"aud_{tag}_{i}"])
            close(r.sigt, g[f"torso_{tag}_{i}"])
    close(R.compute(states, scene, (6, 5, 4, 8)).sig, g["aud_smo_5_len6"])
    for case in ((8, 0, 8, 8), (8, 7, 8, 8)):
        close(R.reference(states, scene, case)[0].sigt, g[f"torso_smo_{case[1]}"])


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_gate_accepts_the_float32_gradients(states, scene, case):
    """the gate on the float32 CPU autograd of the correct reference; the flat layout; which networks take part"""
    r64, r32 = R.reference(states, scene, case)
    st = R.case_states(states, case)
    for n in R.NETS:
        part = {"AudNet": True, "ExpNet": True, "AudAttNet": case[2] > 0, "PoseAttNet": case[3] > 0}[n]
        assert (r64.grads[n] is not None) == part
        if part:
            assert r64.grads[n].dtype == torch.float64 and r64.grads[n].shape == R.flat(st[n]).shape
            sl = R.slices(st[n])
            assert sl[0][1] == 0 and all(a[1] + a[2] == b[1] for a, b in zip(sl, sl[1:])) and sl[-1][1] + sl[-1][2] == R.flat(st[n]).numel()
            assert all(float(r64.grads[n][o:o + k].abs().max()) > 0 for _, o, k in sl)      # no tensor the gate could not see
    bad, worst = R.gate_case(r32.grads, states, scene, case)
    assert not bad and worst <= 1.0 / R.GATE_FACTOR + 1e-12
    # the float64 gradients themselves, and the switchable restatement without a switch: the oracle
    bad, worst = R.gate_case(r64.grads, states, scene, case)
    assert not bad and worst == 0.0
    own = R.compute(states, scene, case, oracle=False)
    torch.testing.assert_close(own.sig, r64.sig, rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(own.sigt, r64.sigt, rtol=1e-13, atol=1e-15)
    for n in R.NETS:
        assert (own.grads[n] is None) == (r64.grads[n] is None)
        if own.grads[n] is not None:
            scale = float(r64.grads[n].abs().max())
            assert float((own.grads[n] - r64.grads[n]).abs().max()) <= 1e-12 * scale


def test_gate_sizes_the_tolerance_from_the_reference():
    g64 = torch.tensor([1.0, -2.0, 0.5], dtype=torch.float64)
    g32 = g64.float()
    tol = 8 * 2.0 ** -23 * 2.0                       # no float32 error: the format's floor at the largest entry
    assert R.tolerance(g64, g32) == tol
    assert R.gate_tensor(g64 + torch.tensor([0, 0, 0.99 * tol]), g64, g32)[2]
    assert not R.gate_tensor(g64 + torch.tensor([0, 0, 1.01 * tol]), g64, g32)[2]
    g32 = (g64 + torch.tensor([3e-6, 0, 0])).float()
    assert abs(R.tolerance(g64, g32) - 8 * 3e-6) < 1e-6 * 8 * 3e-6 + 8 * 2.0 ** -24
    assert not R.gate_tensor(torch.tensor([1.0, float("nan"), 0.5]), g64, g32)[2]
    # a network's error level: the median of e32 / max|g64| over its tensors holds up the tolerance of a tensor whose own
    # draw fell under it (a one-entry tensor), and moves no tolerance above it
    r64 = torch.tensor([1.0, 2.0, 4.0, 0.5, 3.0], dtype=torch.float64)
    r32 = (r64 + torch.tensor([2e-6, 4e-6, 1e-5, 0.0, 6e-6], dtype=torch.float64))
    sl = [("a", 0, 2), ("b", 2, 1), ("c", 3, 1), ("d", 4, 1)]            # e32 / max: 2e-6, 2.5e-6, 0, 2e-6 -> level 2e-6
    near = lambda a, b: abs(a - b) <= 1e-9 * abs(b)
    assert near(R.error_level(r64, r32, sl), 2e-6)
    res = {k: (tol, own) for k, _, tol, _, own in R.gate(r64.float(), r64, r32, sl)}
    assert near(res["c"][0], 8 * 2e-6 * 0.5) and res["c"][1] == 8 * 2.0 ** -23 * 0.5
    assert near(res["b"][0], 8e-5) and all(near(res[k][0], res[k][1]) for k in "abd")
    z = torch.zeros(4, dtype=torch.float64)          # an exactly zero reference: exactly zero
    assert R.gate_tensor(torch.zeros(4), z, z.float())[2] and not R.gate_tensor(torch.tensor([0, 0, 1e-30, 0]), z, z.float())[2]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_gate_rejects_mutant(states, scene, mutant):
    """Each wrong reference, in float64 (nothing but the mutation separates it from the reference), on every case whose
    gradients it changes: the gate fails on at least one tensor."""
    cases = [c for c in R.CASES if R.mutant_applies(mutant, c)]
    assert len(cases) >= 3, cases
    for case in cases:
        m = R.compute(states, scene, case, mutant=mutant, oracle=False)
        bad, worst = R.gate_case(m.grads, states, scene, case)
        print(f"{mutant} {R.case_id(case)}: {len(bad)} tensors rejected, worst error / tolerance {worst:.3g}")
        assert bad, (mutant, case)
        assert worst >= 100.0, (mutant, case, worst)        # rejected with room: not a near miss of the gate
