"""Host-side checks of the gradient guard (include/dfanerf.h: dfn_grad_stats, dfn_adam_multi_guarded; optim.HipAdam's
max_grad_norm / skip_nonfinite; run_nerf.make_adam's environment switches), no GPU: names, refusals before any device work,
constructor and environment parsing, and the documented accumulation order against float64."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import grad_guard_ref as R
from conftest import ROOT
from dfanerf import _lib

ONE = C.c_void_p(4096)        # a non-null address that is never dereferenced: every call below is refused before it would be
N = None
L = _lib.lib
NEW = ("dfn_grad_stats_floats", "dfn_grad_stats", "dfn_adam_multi_guarded")


def _declared_arg_count(hdr, name):
    m = re.search(r"\b(?:int|long)\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/dfanerf.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_library_and_exports_agree_on_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "dfanerf.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, n_args in zip(NEW, (1, 10, 12)):
        assert name in _lib.EXPORTS and hasattr(raw, name), name
        assert _declared_arg_count(hdr, name) == len(getattr(L, name).argtypes) == n_args, name
    # the guarded step is dfn_adam_multi plus (t_host, stats)
    assert _declared_arg_count(hdr, "dfn_adam_multi") + 2 == _declared_arg_count(hdr, "dfn_adam_multi_guarded")
    # the record: the header's fields in the header's order, 32 bytes
    body = hdr[hdr.index("typedef struct DfnGradStats {"):hdr.index("} DfnGradStats;")]
    fields = re.findall(r"^\s*(?:double|float|int32_t)\s+(\w+);", body, re.M)
    assert fields == [f[0] for f in _lib.DfnGradStats._fields_] and C.sizeof(_lib.DfnGradStats) == 32
    assert fields[:6] == ["sumsq", "norm", "nonfinite", "clip_coef", "skip", "skipped_total"]
    # the comment states the rules and cites the reference lines it stands in for
    doc = hdr[hdr.index("---- gradient guard"):hdr.index("/* ---- Decoder.forward on explicit points")]
    for word in ("MAIN:916-931", "HELP:5", "FIXED ORDER", "no floating-point atomics", "index order in\n *     double",
                 "NOT\n * scaled", "t_eff = t_host - stats->skipped_total", "max_norm / (norm + 1e-6f)", "clip_grad_norm_"):
        assert word in doc, word


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    def refused(rc, name, word=None):
        err = L.dfn_last_error().decode()
        assert rc == -1 and err.startswith(name + ":") and (word is None or word in err), (rc, err)

    stats = (ONE, ONE, 4, 0, 1, 0.0, 1, ONE, ONE, N)
    for k, word in ((0, "table"), (1, "table"), (7, "workspace"), (8, "stats record")):
        a = list(stats)
        a[k] = N
        refused(L.dfn_grad_stats(*a), "dfn_grad_stats", word)
    for n in (0, -3):
        a = list(stats)
        a[2] = n
        refused(L.dfn_grad_stats(*a), "dfn_grad_stats", "n_chunks")
    a = list(stats)
    a[3] = -1
    refused(L.dfn_grad_stats(*a), "dfn_grad_stats", "chunk_base")
    a = list(stats)
    a[5] = float("nan")
    refused(L.dfn_grad_stats(*a), "dfn_grad_stats", "max_norm")

    adam = (ONE, ONE, 4, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, 1, ONE, N)
    for k, word in ((0, "table"), (1, "table"), (10, "stats record")):
        a = list(adam)
        a[k] = N
        refused(L.dfn_adam_multi_guarded(*a), "dfn_adam_multi_guarded", word)
    for n in (0, -1):
        a = list(adam)
        a[2] = n
        refused(L.dfn_adam_multi_guarded(*a), "dfn_adam_multi_guarded", "n_chunks")
    a = list(adam)
    a[7] = 0.0                                   # t = 0: bias_c1 = 0, as dfn_adam_multi
    refused(L.dfn_adam_multi_guarded(*a), "dfn_adam_multi_guarded")
    a = list(adam)
    a[9] = 0
    refused(L.dfn_adam_multi_guarded(*a), "dfn_adam_multi_guarded", "t_host")

    for n in (0, -5):
        refused(L.dfn_grad_stats_floats(n), "dfn_grad_stats_floats", "n_chunks")
    assert L.dfn_grad_stats_floats(1) == 2 and L.dfn_grad_stats_floats(R.N_CHUNKS) == 2 * R.N_CHUNKS == 2 * 714


def test_hip_adam_constructor_checks():
    from dfanerf.optim import HipAdam
    ps = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (-1.0, -1e-9, float("nan"), float("inf"), float("-inf"), "1.0", True):
        with pytest.raises(ValueError, match="max_grad_norm"):
            HipAdam(ps, lr=1e-3, max_grad_norm=bad)
    o = HipAdam(ps, lr=1e-3)
    assert o.max_grad_norm is None and o.skip_nonfinite is False and not o._guarded and o._gs is None
    with pytest.raises(ValueError, match="guard is off"):
        o.grad_stats()
    for kw in ({"max_grad_norm": 2}, {"skip_nonfinite": True}, {"max_grad_norm": 0.5, "skip_nonfinite": True}):
        o = HipAdam(ps, lr=1e-3, **kw)
        assert o._guarded and o.max_grad_norm == kw.get("max_grad_norm") and o.skip_nonfinite == kw.get("skip_nonfinite", False)
        assert o.grad_stats() == {"norm": 0.0, "nonfinite": 0, "clip_coef": 1.0, "skipped_total": 0}      # before the first step
        # what HipAdam would hand to torch's own step() is refused with the guard on, not run unguarded
        ps[0].grad = torch.ones(3)
        o.param_groups[0]["weight_decay"] = 0.1
        with pytest.raises(ValueError, match="unguarded"):
            o.step()
        o.param_groups[0]["weight_decay"] = 0
        o.param_groups[0]["amsgrad"] = True
        with pytest.raises(ValueError, match="unguarded"):
            o.step()
        o.param_groups[0]["amsgrad"] = False
        with pytest.raises(ValueError, match="unguarded"):     # a tensor the kernels do not take (here: not on the GPU)
            o.step()
        assert torch.equal(ps[0].detach(), torch.zeros(3))
        ps[0].grad = None


class _FakeParam:
    is_cuda = True


def test_make_adam_reads_the_guard_from_the_environment(monkeypatch):
    from dfanerf import optim, run_nerf
    seen = []

    def fake(params, **kw):
        seen.append(kw)
        return "opt"

    monkeypatch.setattr(optim, "HipAdam", fake)
    ps = [_FakeParam()]
    monkeypatch.delenv("DFN_GRAD_GUARD", raising=False)
    monkeypatch.delenv("DFN_MAX_GRAD_NORM", raising=False)
    assert run_nerf.make_adam(ps, 5e-4) == "opt"
    assert seen[-1] == {"lr": 5e-4, "betas": (0.9, 0.999)}                     # unset: off, HipAdam's defaults
    monkeypatch.setenv("DFN_GRAD_GUARD", "1")
    monkeypatch.setenv("DFN_MAX_GRAD_NORM", "0.5")
    run_nerf.make_adam(ps, 5e-4)
    assert seen[-1] == {"lr": 5e-4, "betas": (0.9, 0.999), "skip_nonfinite": True, "max_grad_norm": 0.5}
    monkeypatch.setenv("DFN_GRAD_GUARD", "0")
    run_nerf.make_adam(ps, 5e-4)
    assert seen[-1] == {"lr": 5e-4, "betas": (0.9, 0.999), "max_grad_norm": 0.5}
    n = len(seen)
    for name, val in (("DFN_MAX_GRAD_NORM", "abc"), ("DFN_MAX_GRAD_NORM", "-1"), ("DFN_MAX_GRAD_NORM", "nan"),
                      ("DFN_GRAD_GUARD", "yes")):
        monkeypatch.setenv("DFN_GRAD_GUARD", "1")
        monkeypatch.setenv("DFN_MAX_GRAD_NORM", "0.5")
        monkeypatch.setenv(name, val)
        with pytest.raises(ValueError, match=name):
            run_nerf.make_adam(ps, 5e-4)
    assert len(seen) == n
    # the flag tables stay as they are: the guard has no command-line flag
    assert not any("grad" in str(f).lower() and "guard" in str(f).lower() for f in run_nerf._EXTRA_FLAGS)


def test_documented_accumulation_order_stays_inside_the_tolerance():
    """The reference alone, on the CPU: the documented order (grad_guard_ref.chunk_partials / ordered_sumsq) on the GPU test's
    tensor list, scale and distribution - randn * 1e-3 per tensor; the GPU test draws its values from a device generator, whose
    stream a CPU generator does not reproduce, and checks the kernel bit for bit against this same restatement on the values
    it drew - differs from the float64 norm by less than a quarter of the GPU test's tolerance."""
    g = torch.Generator().manual_seed(1)
    grads = [(torch.randn(s, generator=g) * 1e-3).numpy() for s in R.SHAPES]
    parts = R.chunk_partials(grads)
    assert parts.shape == (R.N_CHUNKS,) and parts.dtype == np.float32
    ref = R.norm64(grads)
    got = float(np.float32(np.sqrt(R.ordered_sumsq(grads))))
    err = abs(got - ref) / ref
    print(f"documented order vs float64: rel.err {err:.2e} (bound {R.NORM_RTOL / 4:.1e})")
    assert err < R.NORM_RTOL / 4
    # the order is a property of the restatement too: the chunks of a tensor do not depend on its neighbours ...
    assert np.array_equal(R.chunk_partials(grads[::-1]), np.concatenate([R.chunk_partials([x]) for x in grads[::-1]]))
    # ... a one-element tensor's partial is its square, exactly; an overflowing square and a NaN stay what they are
    assert R.chunk_partials([np.float32([3.0])])[0] == np.float32(9.0)
    assert np.isinf(R.ordered_sumsq([np.float32([1e30, 1.0])])) and np.isnan(R.ordered_sumsq([np.float32([np.nan, 1.0])]))
