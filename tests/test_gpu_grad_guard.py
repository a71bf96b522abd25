"""GPU tests of the gradient guard: dfn_grad_stats (total norm in a fixed order, non-finite count, the decision) and
dfn_adam_multi_guarded through optim.HipAdam(max_grad_norm=, skip_nonfinite=) - against float64, torch.optim.Adam,
torch.nn.utils.clip_grad_norm_, the unguarded HipAdam (bit for bit) and, in the fused training step, against the same
steps with the guard off.  A NaN in a gradient buffer is an ordinary float on this path: nothing here provokes a fault."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import grad_guard_ref as R
from dfanerf import synth   # noqa: F401  (the package, before anything that needs the library)

pytestmark = pytest.mark.gpu

NORM_RTOL = R.NORM_RTOL     # derivation: grad_guard_ref's docstring (the documented order: 12 roundings per element path)


def t(x):
    return torch.from_numpy(np.asarray(x))


@pytest.fixture(scope="module")
def base():
    """Parameters (CPU) and the gradients of the tests (device generator, seed 1, randn * 1e-3) - made once, never changed."""
    g = torch.Generator().manual_seed(0)
    params = [torch.randn(*s, generator=g) for s in R.SHAPES]
    gen = torch.Generator(device="cuda").manual_seed(1)
    grads = [torch.randn(s, device="cuda", generator=gen) * 1e-3 for s in R.SHAPES]
    return params, grads


def _params(base):
    return [torch.nn.Parameter(p.clone().cuda()) for p in base[0]]


def _set_grads(ps, grads, scale=1.0):
    for p, g in zip(ps, grads):
        if p.grad is None:
            p.grad = g * scale if scale != 1.0 else g.clone()
        else:
            p.grad.copy_(g * scale if scale != 1.0 else g)


def _table(tensors):
    """items / chunks of dfn_adam_multi for `tensors` as gradients (param / moments: never touched by dfn_grad_stats)"""
    items = np.zeros((len(tensors), 5), np.int64)
    chunks = []
    for i, g in enumerate(tensors):
        items[i] = (0, g.data_ptr(), 0, 0, g.numel())
        chunks.extend((i, k) for k in range(-(-g.numel() // R.CHUNK)))
    return t(items).cuda(), t(np.asarray(chunks, np.int32).reshape(-1, 2)).cuda(), len(chunks)


def _stats(tensors, max_norm=0.0, skip_nonfinite=1, rec=None):
    from dfanerf._lib import DfnGradStats, check, lib
    items, chunks, n = _table(tensors)
    ws = torch.empty(lib.dfn_grad_stats_floats(n), device="cuda")
    rec = torch.zeros(8, dtype=torch.int32, device="cuda") if rec is None else rec
    check(lib.dfn_grad_stats(items.data_ptr(), chunks.data_ptr(), n, 0, 1, max_norm, skip_nonfinite, ws.data_ptr(), rec.data_ptr(),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dfn_grad_stats")
    torch.cuda.synchronize()
    return DfnGradStats.from_buffer_copy(rec.cpu().numpy().tobytes()), ws.cpu().numpy()[0::2].copy()


def _same(a, oa, b, ob, tol=1e-5):
    """the gates of test_hip_adam_matches_torch_adam, unchanged"""
    for p, q in zip(a, b):
        assert torch.allclose(p, q, rtol=tol, atol=1e-6), (p - q).abs().max().item()
        sa, sb = oa.state[p], ob.state[q]
        if len(sb):
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.allclose(sa[k], sb[k], rtol=tol, atol=1e-6 * float(sb[k].abs().max())), k


def _snapshot(ps, opt):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]


def _bit_equal(s0, s1):
    return all(torch.equal(x, y) for a, b in zip(s0, s1) for x, y in zip(a, b))


def test_norm_against_float64(base):
    _, grads = base
    host = [g.cpu().numpy() for g in grads]
    ref = R.norm64(host)
    st, parts = _stats(grads)
    err = abs(st.norm - ref) / ref
    print(f"norm {st.norm:.9g} vs float64 {ref:.9g}: rel.err {err:.2e} (gate {NORM_RTOL:.0e})")
    assert err <= NORM_RTOL
    assert st.nonfinite == 0 and st.skip == 0 and st.skipped_total == 0 and st.clip_coef == 1.0
    assert abs(st.norm - np.float32(math.sqrt(st.sumsq))) <= np.spacing(np.float32(st.norm))     # (float)sqrt(sumsq)
    # ... and the kernel IS the documented order: every chunk's partial and the double sum, bit for bit
    assert parts.shape == (R.N_CHUNKS,) and np.array_equal(parts, R.chunk_partials(host))
    assert st.sumsq == R.ordered_sumsq(host)
    # the decision's formula (torch.nn.utils.clip_grad_norm_), in f32 as documented
    for max_norm in (ref * 0.5, ref * 2.0):
        st2, _ = _stats(grads, max_norm=max_norm)
        want = min(np.float32(1.0), np.float32(max_norm) / (np.float32(st2.norm) + np.float32(1e-6)))
        assert abs(st2.clip_coef - want) <= np.spacing(want) and (st2.clip_coef < 1.0) == (max_norm < ref), (st2.clip_coef, want)
    st3, _ = _stats(grads, max_norm=0.0)
    assert st3.clip_coef == 1.0                               # max_norm <= 0: no clipping, exactly 1.0f


def test_stats_are_reproducible(base):
    """Two calls on the same gradients: every field bit-equal, sumsq included.  With the tensors listed in reverse order in a
    second table the documented order allows this much: each chunk's partial is the same bits (a chunk's sum does not depend on
    where its tensor stands), the partials are then added in the NEW index order in double - so sumsq agrees to double
    rounding (each order is within n_chunks * 2^-53 relative of the exact sum), not necessarily bit for bit, and the f32 norm
    within one ulp."""
    _, grads = base
    a, pa = _stats(grads)
    b, pb = _stats(grads)
    assert bytes(a) == bytes(b) and np.array_equal(pa, pb)
    r, pr = _stats(grads[::-1])
    by_tensor = np.cumsum([0] + [-(-g.numel() // R.CHUNK) for g in grads])
    fwd = [pa[by_tensor[i]:by_tensor[i + 1]] for i in range(len(grads))]
    assert np.array_equal(pr, np.concatenate(fwd[::-1]))
    assert abs(r.sumsq - a.sumsq) <= 2 * R.N_CHUNKS * 2.0 ** -53 * a.sumsq
    assert abs(r.norm - a.norm) <= np.spacing(np.float32(a.norm)) and r.nonfinite == a.nonfinite == 0


@pytest.mark.parametrize("max_grad_norm", [None, 1e9])
def test_guard_on_nothing_triggers_is_bitwise_the_plain_step(base, max_grad_norm):
    from dfanerf.optim import HipAdam
    _, grads = base
    a, b = _params(base), _params(base)
    oa = HipAdam(a, lr=5e-4, skip_nonfinite=True, max_grad_norm=max_grad_norm)
    ob = HipAdam(b, lr=5e-4)
    for it in range(3):
        _set_grads(a, grads, 1.0 + it)
        _set_grads(b, grads, 1.0 + it)
        for o in (oa, ob):
            o.param_groups[0]["lr"] = 5e-4 * 0.9 ** it
            o.step()
        st = oa.grad_stats()
        assert st["clip_coef"] == 1.0 and st["nonfinite"] == 0 and st["skipped_total"] == 0 and st["norm"] > 0
    torch.cuda.synchronize()
    assert _bit_equal(_snapshot(a, oa), _snapshot(b, ob))
    assert ob._gs is None                                                        # the plain step allocates nothing new
    assert [float(oa.state_dict()["state"][k]["step"]) for k in range(len(a))] == [3.0] * len(a)


def test_clipping_matches_torch(base):
    from dfanerf.optim import HipAdam
    _, grads = base
    host = [g.cpu().numpy() for g in grads]
    n0 = R.norm64(host)
    scales = [0.1 + it for it in range(5)]
    max_norm = n0 * 2.0                     # between the smallest (0.1 n0) and the largest (4.1 n0) of the five norms
    a, b, c = _params(base), _params(base), _params(base)
    oa = HipAdam(a, lr=5e-4, max_grad_norm=max_norm)
    ob, oc = torch.optim.Adam(b, lr=5e-4), torch.optim.Adam(c, lr=5e-4)
    clipped = []
    for it, sc in enumerate(scales):
        gs = [g * sc for g in grads]
        n64 = R.norm64([x.cpu().numpy() for x in gs])
        coef = np.float32(min(1.0, max_norm / (n64 + 1e-6)))
        _set_grads(a, gs)                                     # (the same buffers every step: the cached table is reused)
        for q, r, g in zip(b, c, gs):
            q.grad, r.grad = g * float(coef), g.clone()
        keep = [p.grad.clone() for p in a]
        torch.nn.utils.clip_grad_norm_(c, max_norm)
        for o in (oa, ob, oc):
            o.param_groups[0]["lr"] = 5e-4 * 0.9 ** it
            o.step()
        st = oa.grad_stats()
        # (the coefficient: the norm's tolerance plus the f32 roundings of the sum, the quotient and the casts)
        assert abs(st["norm"] - n64) <= NORM_RTOL * n64, (st, n64)
        assert abs(st["clip_coef"] - float(coef)) <= (NORM_RTOL + 4 * 2.0 ** -24) * float(coef), (st, coef)
        clipped.append(st["clip_coef"] < 1.0)
        assert all(torch.equal(p.grad, k) for p, k in zip(a, keep))             # the gradient buffers are only read
        _same(a, oa, b, ob)
        _same(a, oa, c, oc)
    assert clipped == [False, False, True, True, True]                           # both kinds occur


def _inject(kind, grads):
    g = [x.clone() for x in grads]
    if kind == "nan_last":
        g[-1].view(-1)[-1] = float("nan")                    # last element of the last tensor
    elif kind == "nan_partial_chunk":
        g[7].view(-1)[-1] = float("nan")                     # last element of the last, partial chunk (3 elements) of the big tensor
    elif kind == "inf_first":
        g[0].view(-1)[0] = float("inf")
    elif kind == "overflow":
        g[6].view(-1)[4321] = 1e30                           # finite; its square overflows the f32 partial
    return g


@pytest.mark.parametrize("kind", ["nan_last", "nan_partial_chunk", "inf_first", "overflow"])
def test_nonfinite_step_is_skipped(base, kind):
    from dfanerf.optim import HipAdam
    _, grads = base
    # (64, 64) is the last tensor of the list: a whole number of chunks.  The NaN case the guard must not miss is a partial last
    # chunk, so one variant lists the tensors with the 3-element-tail tensor last
    order = list(range(len(grads)))
    if kind == "nan_partial_chunk":
        order = [i for i in order if i != 7] + [7]
    pbase = ([base[0][i] for i in order], None)
    gr = [grads[i] for i in order]
    bad = [_inject(kind, grads)[i] for i in order]
    a, b, c = _params(pbase), _params(pbase), _params(pbase)
    oa = HipAdam(a, lr=5e-4, skip_nonfinite=True)
    ob = torch.optim.Adam(b, lr=5e-4)
    oc = HipAdam(c, lr=5e-4)                                  # unguarded: the injection reaches the update
    # step 1
    for ps, o in ((a, oa), (b, ob), (c, oc)):
        _set_grads(ps, gr)
        o.step()
    s1 = _snapshot(a, oa)
    # step 2: one bad value
    _set_grads(a, bad)
    oa.step()
    st = oa.grad_stats()
    assert _bit_equal(_snapshot(a, oa), s1)
    assert st["skipped_total"] == 1 and st["nonfinite"] >= 1 and not math.isfinite(st["norm"])
    _set_grads(c, bad)
    oc.step()
    torch.cuda.synchronize()
    # ... and the guard is what stops it: unguarded, the same step writes NaN into the parameters (1e30: an Inf into exp_avg_sq,
    # the update of that element is m / inf = 0)
    if kind == "overflow":
        assert any(bool(torch.isinf(oc.state[p]["exp_avg_sq"]).any()) for p in c)
    else:
        assert any(bool(torch.isnan(p).any()) for p in c)
    # step 3
    for ps, o in ((a, oa), (b, ob)):
        _set_grads(ps, gr, 2.0)
        o.step()
    st = oa.grad_stats()
    assert st["skipped_total"] == 1 and st["nonfinite"] == 0
    _same(a, oa, b, ob)                                                          # torch Adam that took steps 1 and 3 only
    sd = oa.state_dict()["state"]
    assert [float(sd[k]["step"]) for k in range(len(a))] == [2.0] * len(a)
    # the record is rebuilt with the table: new gradient tensors, the counts carry on without the skipped step
    for ps, o in ((a, oa), (b, ob)):
        for p, g in zip(ps, gr):
            p.grad = g * 0.5
        o.step()
    _same(a, oa, b, ob)
    assert oa.grad_stats()["skipped_total"] == 1
    assert [float(oa.state_dict()["state"][k]["step"]) for k in range(len(a))] == [3.0] * len(a)


def test_two_step_counts_one_norm_one_skip(base):
    """A tensor without gradient for two steps leaves two buckets (two launch tables): ONE norm over both, one skip stops both
    and moves skipped_total by one."""
    from dfanerf.optim import HipAdam
    _, grads = base
    a, b = _params(base), _params(base)
    oa = HipAdam(a, lr=5e-4, skip_nonfinite=True, max_grad_norm=1e9)
    ob = torch.optim.Adam(b, lr=5e-4)

    def step(gs, skip=None, ref=True):
        for k, (p, q, g) in enumerate(zip(a, b, gs)):
            p.grad, q.grad = (None, None) if k == skip else (g.clone(), g.clone())
        oa.step()
        if ref:
            ob.step()

    step(grads, skip=2)
    step(grads, skip=2)
    step(grads)
    assert sorted(bk["t"] for bk in oa._cache[0]["buckets"]) == [1, 3]
    st = oa.grad_stats()
    n64 = R.norm64([g.cpu().numpy() for g in grads])
    assert abs(st["norm"] - n64) <= NORM_RTOL * n64 and st["skipped_total"] == 0
    _same(a, oa, b, ob)
    s0 = _snapshot(a, oa)
    bad = [g.clone() for g in grads]
    bad[2].view(-1)[7] = float("nan")                         # in the one-tensor bucket
    _set_grads(a, bad)
    oa.step()
    assert _bit_equal(_snapshot(a, oa), s0) and oa.grad_stats()["skipped_total"] == 1
    bad = [g.clone() for g in grads]
    bad[5].view(-1)[2048] = float("-inf")                     # in the other bucket
    _set_grads(a, bad)
    oa.step()
    st = oa.grad_stats()
    assert _bit_equal(_snapshot(a, oa), s0) and st["skipped_total"] == 2 and st["nonfinite"] == 1
    _set_grads(a, grads)
    _set_grads(b, grads)
    oa.step()
    ob.step()
    _same(a, oa, b, ob)
    sd = oa.state_dict()["state"]
    assert [float(sd[k]["step"]) for k in range(len(a))] == [2.0 if k == 2 else 4.0 for k in range(len(a))]


@pytest.mark.parametrize("tier", ["f32", "bf16"])
def test_guard_in_the_fused_training_step(states, scene, latents, golden, monkeypatch, tier):
    """The fused two-field step (256 pixels, all five networks, optimizers from make_adam, the conditioning networks' Adam on
    their own streams): two steps with DFN_GRAD_GUARD=1 DFN_MAX_GRAD_NORM=1e9 end in the parameters of two steps with neither,
    bit for bit, and the decoder's norm is the float64 norm of its gradients.  A wrong stream or a missing wait in front of the
    stats launch shows here."""
    from dfanerf import nets, run_nerf, training
    g = golden("g8_train_step")
    dev = torch.device("cuda")
    args = run_nerf.config_parser().parse_args(
        "--expname t --concate_bg --N_rand=256 --sample_rate=0 --smo_size=4 --smo_torse_size 8 --use_et_embed "
        "--dim_signal=96 --dim_aud=96 --n_object=1 --use_deformation_field --noexp_iters 400000".split())
    H, W = scene["H"], scene["W"]
    ds = [{"auds": t(scene["aud"]).to(dev), "exp": t(scene["exp"]).to(dev), "poses": t(scene["poses"]).to(dev),
           "bc_img": (t(scene["bg"]).float() / 255.0).to(dev), "hwfcxy": [H, W, scene["focal"], scene["cx"], scene["cy"]],
           "near": 0.3, "far": 0.9}]
    sel = g["sel_yx"]
    zs, za = [t(v).to(dev) for v in latents]
    embed_fn, _ = nets.get_embedder(3, 0)
    gen = torch.Generator(device=dev).manual_seed(3)
    tgts = [torch.rand(sel.shape[0], 3, device=dev, generator=gen) for _ in range(2)]

    def run(guard):
        for name, val in (("DFN_GRAD_GUARD", "1"), ("DFN_MAX_GRAD_NORM", "1e9")):
            if guard:
                monkeypatch.setenv(name, val)
            else:
                monkeypatch.delenv(name, raising=False)
        from dfanerf.decoder import Decoder
        mods = {"decoder": Decoder(z_dim=256, hidden_size=256, dim_signal=96, use_deformation_field=True),
                "AudNet": nets.AudioNet_W2L(), "ExpNet": nets.ExpressionEnc(), "AudAttNet": nets.AudioAttNet(96, 4),
                "PoseAttNet": nets.AudioAttNet(42, 8)}
        for k, m in mods.items():
            m.load_state_dict({kk: t(v) for kk, v in states[k].items()})
            m.to(dev)
        opts = {k: run_nerf.make_adam(m.parameters(), 5e-4) for k, m in mods.items()}
        assert all(o._guarded == guard for o in opts.values())
        buf = training.TrainBuffers(tier, sel.shape[0], dev)
        buf.signal_trainer = training.SignalTrainer(mods["AudNet"], mods["ExpNet"], mods["AudAttNet"], mods["PoseAttNet"],
                                                    ds[0]["auds"], ds[0]["exp"], ds[0]["poses"])
        buf.signal_trainer.adopt_optimizers(opts)
        for k in range(2):
            loss, *_ = run_nerf.train_step_loss_hip(mods, ds, 0, 2 + k, sel, tgts[k], tgts[k], zs, za, 300000, args,
                                                    scene["aud"].shape[0], embed_fn, ds[0]["poses"][0], buf)
            for o in opts.values():
                o.zero_grad()
            loss.backward()
            run_nerf.optimizer_steps(opts, 300000, args)
        buf.signal_trainer.join()
        torch.cuda.synchronize()
        return mods, opts

    m0, _ = run(False)
    m1, o1 = run(True)
    n_moved = 0
    for tag in m0:
        for (k, p), (_, q) in zip(m0[tag].named_parameters(), m1[tag].named_parameters()):
            assert torch.equal(p, q), (tag, k)
            n_moved += int((p.detach().cpu() != t(states[tag][k])).any())
    assert n_moved > 20                                       # the steps did train
    st = o1["decoder"].grad_stats()
    n64 = R.norm64([p.grad.cpu().numpy() for p in m1["decoder"].parameters() if p.grad is not None])
    print(f"decoder norm {st['norm']:.9g} vs float64 {n64:.9g}")
    assert n64 > 0 and abs(st["norm"] - n64) <= NORM_RTOL * n64
    assert st["nonfinite"] == 0 and st["clip_coef"] == 1.0 and st["skipped_total"] == 0
    for k in ("AudNet", "AudAttNet", "PoseAttNet"):           # guarded on their own streams, over their own parameters
        s = o1[k].grad_stats()
        ref = R.norm64([p.grad.cpu().numpy() for p in m1[k].parameters() if p.grad is not None])
        assert s["skipped_total"] == 0 and abs(s["norm"] - ref) <= NORM_RTOL * ref, (k, s, ref)
