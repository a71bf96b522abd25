"""GPU tests of the training step's per-ray opacity and expected depth: dfn_composite_stats (composite_stats_kernel),
dfn_composite_bwd_stats (the <.., STATS> instantiations of the two compositing backward kernels) and
training.render_train(want_stats=True).

  1. the kernels alone on random samples: stats against the oracle's weights and - bit for bit - against the numpy restatement of the
     documented summation order FED THE KERNELS' OWN WEIGHTS (the restatement does not reproduce expf: the weights are read out of the
     existing compositing backward, whose d colour of a unit d_rgb is the weight itself - see _kernel_weights); dsamples and d_norm of
     the backward against autograd through integrate_fields, with and without a colour gradient;
  2. nothing moved: d_stats = 0 gives the existing family's outputs, a loss that ignores stats gives the plain step, two runs agree;
  3. the whole f32 step on the blend decoder against the oracle's autograd, and on pinhole rays that require grad;
  4. the bf16 tier: the kernels on that tier's recorded samples, and ten Adam steps on the stats loss."""
import ctypes as C

import numpy as np
import pytest
import torch

import blend_scene as B
import dfa_oracle as O
import train_stats_ref as R
from test_gpu_train_hier import _decoder, _signals, t
from test_gpu_train_rays import _assert_same_step, _per_ray_coarse_z, _pixels, _pinhole_rays, _random_rays, _random_samples, _rays_frame

pytestmark = pytest.mark.gpu

N = R.N_RAYS
NEAR, FAR = 0.3, 0.9


def _p(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(*arrays):
    return [None if a is None else t(a).cuda().contiguous() for a in arrays]


def rel_err(a, b):
    a, b = a.detach().double().reshape(-1).cpu(), b.detach().double().reshape(-1).cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


# ---- 1. the kernels alone ---------------------------------------------------------------------------------------------------------------
class Case:
    """96 rays of random raw samples (with the empty-field block), random sorted depths and a random evaluation order in the
    hierarchical step - the set-up of test_composite_backward_hier_vs_autograd - on pixel ids or on rays with per-ray bounds"""

    def __init__(self, scene, n_coarse, n_fine, concate_bg, last_dist, form, seed=0):
        from dfanerf import engine
        self.nc, self.nf, self.S, self.cbg, self.last, self.form = n_coarse, n_fine, n_coarse + n_fine, concate_bg, last_dist, form
        S = self.S
        self.K = S // 64 if n_fine else (2 if n_coarse == 128 else 1)
        rs = np.random.RandomState(101 + S + seed)
        self.samples = _random_samples(rs, N, S)
        self.bg = rs.uniform(0, 1, size=(N, 3)).astype(np.float32)
        self.z_all = self.ranks = self.rays = self.bounds = self.pix = None
        H, W = scene["H"], scene["W"]
        if form == "rays":
            self.rays = _random_rays(rs, N)
            self.bounds = np.stack([0.3 + rs.uniform(0, 0.05, N), 0.9 - rs.uniform(0, 0.05, N)], 1).astype(np.float32)
            junk = np.full((4, 4), 7.5, np.float32)
            self.frame = lambda: engine.make_frame(3, 5, 1.0, -2.0, 9.0, junk, junk, 5.0, 6.0, last_dist, 11, N, n_coarse, n_fine, 2, concate_bg)
            self.dirs = [t(self.rays[:, 3:6]), t(self.rays[:, 9:12])]
            z = _per_ray_coarse_z(t(self.bounds), n_coarse)
            self.bg_rows = self.bg
        else:
            self.pix = rs.permutation(H * W)[:N].astype(np.int32)
            self.poses = (scene["poses"][3], scene["poses"][0])
            self.frame = lambda poses=self.poses: engine.make_frame(H, W, scene["focal"], scene["cx"], scene["cy"], poses[0], poses[1], NEAR,
                                                                    FAR, last_dist, 0, N, n_coarse, n_fine, 2, concate_bg)
            pl = t(self.pix).long()
            self.dirs = [O.get_rays(H, W, scene["focal"], p[:3, :4], scene["cx"], scene["cy"])[1].reshape(-1, 3)[pl] for p in self.poses]
            z = O.coarse_z(NEAR, FAR, n_coarse)[None].expand(N, n_coarse)
            self.bg_img = rs.uniform(0, 1, size=(H * W, 3)).astype(np.float32)
            self.bg_rows = self.bg_img[self.pix]
        if n_fine:
            zz = np.sort(rs.uniform(0.3, 0.9, size=(N, S)).astype(np.float32), axis=1)
            zz[:, -1] = 0.9
            self.z_all = zz
            self.ranks = np.stack([rs.permutation(S) for _ in range(N)]).astype(np.uint8)     # ranks[r, e] = merged position of point e
            z = t(zz)
            idx = t(self.ranks.astype(np.int64))
            self.inv = torch.empty_like(idx)
            self.inv.scatter_(1, idx, torch.arange(S)[None].expand(N, S))                    # inv[r, m] = evaluation index at position m
        self.z = z.contiguous()
        self.d_h, self.d_c = rs.randn(N, 3).astype(np.float32), rs.randn(N, 3).astype(np.float32)
        self.d_s = rs.randn(N, 4).astype(np.float32)

    def merged(self, x):
        """[N, S, ...] in evaluation order -> depth order"""
        if not self.nf:
            return x
        return torch.gather(x, 1, self.inv.reshape(N, self.S, *([1] * (x.dim() - 2))).expand_as(x))

    def source(self, rays=None, frame=None):
        """(frame, pix_index, rays, bounds) on the device, and the background tensor of the form"""
        fr = frame if frame is not None else self.frame()
        if self.form == "rays":
            RY, BD, BG = _dev(self.rays if rays is None else rays, self.bounds, self.bg)
            return (fr, None, RY, BD), BG
        PIX, BG = _dev(self.pix, self.bg_img)
        return (fr, PIX, None, None), BG

    def stats(self):
        from dfanerf._lib import check, lib
        (fr, PIX, RY, BD), _ = self.source()
        Sd, Z, RK = _dev(self.samples, self.z_all, self.ranks)
        out = torch.full((N, 4), float("nan"), device="cuda")
        check(lib.dfn_composite_stats(C.byref(fr), _p(PIX), _p(RY), _p(BD), _p(Sd), _p(Z), _p(RK), _p(out), _st()), "dfn_composite_stats")
        torch.cuda.synchronize()
        return out.cpu()

    def bwd_stats(self, d_h, d_c, d_s, want_norm=False, zero=None):
        from dfanerf._lib import check, lib
        (fr, PIX, RY, BD), BG = self.source()
        Sd, Z, RK, DH, DC, DS = _dev(self.samples, self.z_all, self.ranks, d_h, d_c, d_s)
        ds = torch.full((N, self.S, 8), float("nan"), device="cuda")
        dn = torch.full((N, 2), float("nan"), device="cuda") if want_norm else None
        check(lib.dfn_composite_bwd_stats(C.byref(fr), _p(PIX), _p(RY), _p(BD), _p(BG), None, _p(Sd), _p(Z), _p(RK), _p(DH), _p(DC), _p(DS),
                                          _p(ds), _p(zero), 0 if zero is None else zero.numel(), _p(dn), _st()), "dfn_composite_bwd_stats")
        torch.cuda.synchronize()
        return ds.cpu(), (None if dn is None else dn.cpu())

    def bwd_family(self, d_h, d_c, samples=None, rays=None, frame=None, want_norm=False, zero=None):
        """the existing entry point of the form: _z / _hier_z, _rays_z / _hier_rays_z, or their _zg forms"""
        from dfanerf._lib import check, lib
        (fr, PIX, RY, BD), BG = self.source(rays, frame)
        Sd, Z, RK, DH, DC = _dev(self.samples if samples is None else samples, self.z_all, self.ranks, d_h, d_c)
        ds = torch.full((N, self.S, 8), float("nan"), device="cuda")
        dn = torch.full((N, 2), float("nan"), device="cuda") if want_norm else None
        hier = (_p(Z), _p(RK)) if self.nf else ()
        src = (_p(RY), _p(BD)) if self.form == "rays" else (_p(PIX),)
        name = "dfn_composite_bwd" + ("_hier" if self.nf else "") + ("_rays" if self.form == "rays" else "") + ("_zg" if want_norm else "_z")
        extra = (_p(dn),) if want_norm else ()
        check(getattr(lib, name)(C.byref(fr), *src, _p(BG), None, _p(Sd), *hier, _p(DH), _p(DC), _p(ds), _p(zero),
                                 0 if zero is None else zero.numel(), *extra, _st()), name)
        torch.cuda.synchronize()
        return ds.cpu(), (None if dn is None else dn.cpu())

    def oracle(self, norms=None, samples=None):
        """integrate_fields on the samples in depth order -> rgb_head, w_head, rgb_com, w_com (norms: leaves in place of |d|)"""
        sm = self.merged(t(self.samples) if samples is None else samples)
        dirs = self.dirs
        if norms is not None:
            dirs = [d / d.norm(dim=-1, keepdim=True) * nr[:, None] for d, nr in zip(self.dirs, norms)]
        return O.integrate_fields(self.z, dirs[0], dirs[1], sm[..., 0], sm[..., 1:4], sm[..., 4], sm[..., 5:8], t(self.bg_rows), self.last,
                                  self.cbg)

    def autograd(self, d_h, d_c, d_s):
        """d samples (evaluation order) and d norms of sum rgb . d_rgb + sum stats . d_stats through integrate_fields"""
        sm = t(self.samples).clone().requires_grad_(True)
        norms = [d.norm(dim=-1).clone().requires_grad_(True) for d in self.dirs]
        rh, wh, rc, wc = self.oracle(norms, sm)
        stats = R.stats_of(wh, wc, self.z, self.cbg)
        ((rh * t(d_h)).sum() + (rc * t(d_c)).sum() + (stats * t(d_s)).sum()).backward()
        return sm.grad.numpy(), torch.stack([norms[0].grad, norms[1].grad], 1).numpy()

    def kernel_weights(self):
        """the weights the compositing backward kernels form, bit for bit, in depth order.  Their d colour_head of sample i is
        w_head_i * d_rgb_head + w_com_i * d_rgb_com * (blend share): with d_rgb_head = (1, 0, 0) and d_rgb_com = 0 that is w_head_i
        itself (the background plane's row stays 0: it is not in FG).  The composite's weights are the head image's of a ray whose
        head density is the composite's summed density sigma_h+ + sigma_t+ (formed here in float32 as the kernels form it: the
        background plane's torso density is 0, and the + 1e-6 there is the kernel's own in both images) and whose head direction
        (rays) / head pose (pixel ids) is the torso's"""
        one = np.zeros((N, 3), np.float32)
        one[:, 0] = 1.0
        nul = np.zeros((N, 3), np.float32)
        w_h = self.merged(self.bwd_family(one, nul)[0])[..., 1].numpy()
        sh, stt = np.maximum(self.samples[..., 0], np.float32(0)), np.maximum(self.samples[..., 4], np.float32(0))
        if self.cbg:
            last = (self.ranks == self.S - 1) if self.nf else (np.arange(self.S)[None] == self.S - 1).repeat(N, 0)
            stt = np.where(last, np.float32(0), stt)
        s2 = self.samples.copy()
        s2[..., 0] = (sh + stt).astype(np.float32)
        s2[..., 4] = -1.0
        if self.form == "rays":
            r2 = self.rays.copy()
            r2[:, 3:6] = r2[:, 9:12]
            w_c = self.bwd_family(one, nul, samples=s2, rays=r2)[0]
        else:
            w_c = self.bwd_family(one, nul, samples=s2, frame=self.frame((self.poses[1], self.poses[1])))[0]
        return w_h, self.merged(w_c)[..., 1].numpy()


COUNTS = R.CONFIGS


@pytest.mark.parametrize("form", ["pix", "rays"])
@pytest.mark.parametrize("last_dist", [1e10, 0.05])
@pytest.mark.parametrize("concate_bg", [True, False])
@pytest.mark.parametrize("n_coarse,n_fine", COUNTS)
def test_stats_kernel_and_its_backward_on_random_samples(scene, n_coarse, n_fine, concate_bg, last_dist, form):
    c = Case(scene, n_coarse, n_fine, concate_bg, last_dist, form)
    S = c.S
    got = c.stats().numpy()
    assert np.isfinite(got).all()
    # (a) against the oracle's weights, at test_gpu_aux.py's f32 gates
    with torch.no_grad():
        _, wh, _, wc = c.oracle()
        ref = R.stats_of(wh, wc, c.z, concate_bg).numpy()
    e_acc, e_dep = np.abs(got[:, [0, 2]] - ref[:, [0, 2]]).max(), np.abs(got[:, [1, 3]] - ref[:, [1, 3]]).max()
    print(f"stats {n_coarse}+{n_fine} bg={concate_bg} last={last_dist:g} {form}: max |acc - oracle| {e_acc:.2e} (gate {S * 2e-6:.1e}), "
          f"max |depth - oracle| {e_dep:.2e} (gate {FAR * S * 2e-6:.1e}); acc_com {ref[:, 2].min():.3f} .. {ref[:, 2].max():.3f}")
    assert e_acc <= S * 2e-6 and e_dep <= FAR * S * 2e-6
    # (b) bit for bit: the documented order on the kernels' own weights (and the forward's depths)
    w_h, w_c = c.kernel_weights()
    fg = slice(0, S - 1) if concate_bg else slice(None)        # (a sanity check: over FG they ARE the weights)
    assert np.abs(w_h - wh.numpy())[:, fg].max() <= 1e-4 and np.abs(w_c - wc.numpy())[:, fg].max() <= 1e-4
    zz = c.z.numpy()
    for b, w in ((0, w_h), (1, w_c)):
        a, d = R.ordered_sums(w, zz, c.K, concate_bg)
        assert np.array_equal(a, got[:, 2 * b]), (b, np.abs(a - got[:, 2 * b]).max())
        assert np.array_equal(d, got[:, 2 * b + 1]), (b, np.abs(d - got[:, 2 * b + 1]).max())
    # (c) the backward: colour + stats, then the stats term alone
    rays = form == "rays"
    for what, d_h, d_c in (("colour + stats", c.d_h, c.d_c), ("stats alone", 0 * c.d_h, 0 * c.d_c)):
        zero = torch.full((1031,), 7.0, device="cuda")
        ds, dn = c.bwd_stats(d_h, d_c, c.d_s, want_norm=rays, zero=zero)
        ref_s, ref_n = c.autograd(d_h, d_c, c.d_s)
        ds = ds.numpy()
        print(f"    {what}: max |d samples - autograd| {np.abs(ds - ref_s).max():.2e} (max |ref| {np.abs(ref_s).max():.2e})" +
              (f", max |d_norm - autograd| {np.abs(dn.numpy() - ref_n).max():.2e} (max |ref| {np.abs(ref_n).max():.2e})" if rays else ""))
        assert np.isfinite(ds).all() and np.abs(ref_s[..., 0]).max() > 0 and np.abs(ref_s[..., 4]).max() > 0
        assert float(zero.abs().max()) == 0.0
        np.testing.assert_allclose(ds, ref_s, atol=2e-5 * np.abs(ref_s).max(), rtol=2e-4)
        if rays:
            assert np.abs(ref_n).max() > 0
            np.testing.assert_allclose(dn.numpy(), ref_n, atol=2e-5 * np.abs(ref_n).max(), rtol=2e-4)
    # two runs give the same bits
    assert np.array_equal(c.stats().numpy(), got)


# ---- 2. nothing moved ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["pix", "rays", "rays+norm"])
@pytest.mark.parametrize("n_coarse,n_fine", COUNTS)
def test_zero_d_stats_gives_the_existing_entry_points_outputs(scene, n_coarse, n_fine, form):
    c = Case(scene, n_coarse, n_fine, True, 1e10, form.split("+")[0], seed=1)
    norm = form == "rays+norm"
    z0, z1 = torch.full((1031,), 7.0, device="cuda"), torch.full((1031,), 7.0, device="cuda")
    ds0, dn0 = c.bwd_family(c.d_h, c.d_c, want_norm=norm, zero=z0)
    ds1, dn1 = c.bwd_stats(c.d_h, c.d_c, np.zeros((N, 4), np.float32), want_norm=norm, zero=z1)
    assert bool(torch.isfinite(ds0).all()) and float(ds0.abs().max()) > 0
    assert torch.equal(ds0, ds1) and torch.equal(z0, z1) and float(z1.abs().max()) == 0.0
    if norm:
        assert torch.equal(dn0, dn1) and float(dn0.abs().max()) > 0
    # ... and a d_stats that is not zero moves them
    ds2, _ = c.bwd_stats(c.d_h, c.d_c, c.d_s, want_norm=norm)
    assert not torch.equal(ds0, ds2)


def _step(dec_state, scene, zs, za, sigs, tier, n_coarse, n_fine, n, frame, bg, loss_fn, pix=None, rays=None, bounds=None, want_stats=True,
          steps=1, lr=0.0):
    """forward + backward through render_train (steps > 1: Adam steps on a fixed batch) -> what the step leaves behind, on the CPU.
    loss_fn(rgb_head, rgb_com, stats or None) -> loss"""
    from dfanerf import training
    dev = torch.device("cuda")
    dec = _decoder({"decoder": dec_state}, dev)
    buf = training.TrainBuffers(tier, n, dev, n_fine=n_fine, n_coarse=n_coarse)
    for a in buf.act + buf.masks:        # (the recorder leaves structural padding untouched: compare like with like)
        a.zero_()
    opt = torch.optim.Adam(dec.parameters(), lr=lr) if steps > 1 else None
    losses = []
    for _ in range(steps):
        sh = sigs[0].to(dev).requires_grad_(True)
        st = sigs[1].to(dev).requires_grad_(True)
        if opt is not None:
            opt.zero_grad(set_to_none=True)
        out = training.render_train(dec, buf, frame, bg, None if pix is None else pix.to(dev, torch.int32), sh, st, zs[:2].to(dev),
                                    za[:2].to(dev), rays=rays, bounds=bounds, want_stats=want_stats)
        assert len(out) == (3 if want_stats else 2)
        loss = loss_fn(out[0], out[1], out[2] if want_stats else None)
        loss.backward()
        losses.append(loss.item())
        if opt is not None:
            opt.step()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.detach().cpu().clone()) for k, p in dec.named_parameters()}
    res = dict(rh=out[0].detach().cpu(), rc=out[1].detach().cpu(), loss=losses[-1], losses=losses, d_sh=sh.grad.cpu(), d_st=st.grad.cpu(),
               grads=grads, samples=buf.samples.cpu(), dsamples=buf.dsamples.cpu(), act=[a.cpu() for a in buf.act],
               masks=[m.cpu() for m in buf.masks], stats=out[2].detach().cpu() if want_stats else None,
               params={k: p.detach().cpu().clone() for k, p in dec.named_parameters()}, buf=buf)
    if n_fine:
        res.update(z=buf.z_all.cpu(), ranks=buf.ranks.cpu())
    return res


@pytest.fixture(scope="module")
def sigs(states, scene):
    return _signals(states, scene)


@pytest.mark.parametrize("tier,n_coarse,n_fine,form", [("f32", 64, 0, "pix"), ("f32", 64, 64, "rays"), ("bf16", 32, 0, "rays"),
                                                        ("bf16", 64, 128, "pix")])
def test_a_loss_that_ignores_stats_leaves_the_step_as_it_was(states, scene, latents, sigs, tier, n_coarse, n_fine, form):
    """want_stats=True with the colour loss alone: every parameter gradient, both signal gradients, both images and everything the step
    records are torch.equal to want_stats=False; with the stats in the loss two runs give identical bits"""
    from test_gpu_train_rays import _plain_frame
    dev = torch.device("cuda")
    n = 48 if n_coarse == 32 else 16
    pix = _pixels(scene, n)
    bg_all = (t(scene["bg"]).float() / 255.0).reshape(-1, 3).to(dev)
    zs, za = [t(v)[0] for v in latents]
    tgt = torch.rand(n, 3, generator=torch.Generator().manual_seed(5)).to(dev)
    if form == "rays":
        kw = dict(rays=_pinhole_rays(scene, pix), frame=_rays_frame(n, n_coarse, n_fine), bg=bg_all[pix.to(dev)].contiguous())
    else:
        kw = dict(pix=pix, frame=_plain_frame(scene, n, n_coarse, n_fine), bg=bg_all)
    colour = lambda rh, rc, s: R.colour_loss(rh, rc, tgt)
    both = lambda rh, rc, s: R.colour_loss(rh, rc, tgt) + R.stats_loss(s, R.matte(n))
    args = (states["decoder"], scene, zs, za, sigs, tier, n_coarse, n_fine, n)
    off = _step(*args, loss_fn=colour, want_stats=False, **kw)
    on = _step(*args, loss_fn=colour, **kw)
    _assert_same_step(off, on, "want_stats, ignored", n_fine > 0)
    assert bool(torch.isfinite(on["stats"]).all()) and float(on["stats"][:, [0, 2]].min()) >= 0.0
    a, b = _step(*args, loss_fn=both, **kw), _step(*args, loss_fn=both, **kw)
    _assert_same_step(a, b, "two runs with a stats loss", n_fine > 0)
    assert torch.equal(a["stats"], b["stats"]) and torch.equal(a["stats"], on["stats"])
    assert not torch.equal(a["dsamples"], on["dsamples"])
    # the pinhole rays of the pixels give the pixel step's stats bit for bit: one kernel, two ray sources
    if form == "rays":
        pk = dict(pix=pix, frame=_plain_frame(scene, n, n_coarse, n_fine), bg=bg_all)
        assert torch.equal(_step(*args, loss_fn=colour, **pk)["stats"], on["stats"])


# ---- 3. the whole step, f32, on the blend decoder ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orc(scene, states, latents, golden):
    return B.Oracle(scene, B.blend_state(states), latents, golden("g7_frame_coarse"), pix=B.ray_indices(scene, N))


def _posenc_c32(p, n_freq, downscale=2.0):
    import math
    p = p / downscale
    out = []
    for i in range(n_freq):
        c = float(np.float32((2 ** i) * math.pi))
        out += [torch.sin(c * p), torch.cos(c * p)]
    return torch.cat(out, -1)


def _oracle_step(orc, z, tgt, m, dt, rays=None):
    """the oracle's autograd of colour MSE + stats loss at depths z: render_fixed_samples' composition with the weights kept
    (blend_scene.Oracle.integrate) -> loss, {decoder gradients}, d sig_head, d sig_torso, d rays [n, 12].  dt float64: the oracle's own
    arithmetic in float64 (blend_scene.oracle_f64: float32 values cast, the encoding's float32 constants kept)"""
    keep = O.posenc
    if dt == torch.float64:
        O.posenc = _posenc_c32
    try:
        c = lambda x: None if x is None else x.to(dt)
        P = {k: v.to(dt).clone().requires_grad_(True) for k, v in orc.P.items()}
        leaves = [c(r).clone().requires_grad_(True) for r in (orc.rays if rays is None else rays)]
        sig, sigt = c(orc.sig[0]).clone().requires_grad_(True), c(orc.sigt).clone().requires_grad_(True)
        zz = c(t(np.asarray(z)))
        s = O._eval_fields(P, *leaves, zz, c(orc.zs), c(orc.za), [sig, None], sigt, 2)
        rh, wh, rc, wc = O.integrate_fields(zz, leaves[1], leaves[3], *s, c(orc.bg))
        loss = R.colour_loss(rh, rc, tgt.to(dt)) + R.stats_loss(R.stats_of(wh, wc, zz), m.to(dt))
        loss.backward()
        return (loss.item(), {k: v.grad for k, v in P.items()}, sig.grad.reshape(-1), sigt.grad.reshape(-1),
                torch.cat([x.grad for x in leaves], 1), R.stats_of(wh, wc, zz).detach())
    finally:
        O.posenc = keep


# tensors that may be gated against the float64 oracle (at 4 x the f32 oracle's own distance from it) where they miss the ordinary gate:
# none has needed it
F64_YARDSTICK = ()


@pytest.mark.parametrize("n_fine", [0, 64])
def test_stats_step_vs_oracle_autograd(orc, scene, latents, golden, n_fine):
    """blend decoder, the 96 rays, f32, coarse 64 and 64 + 64: loss = colour MSE + stats loss against the oracle's autograd at the
    step's own depths, at DESIGN.md 3's f32 gradient gates (test_gpu_blend.py::test_training_step_vs_oracle_autograd); then the same
    step on training.pinhole_rays that require grad."""
    from dfanerf import engine, training
    dev = torch.device("cuda")
    pix = t(orc.pix).long()
    H, W = scene["H"], scene["W"]
    sig_h, sig_t, zs, za = [t(np.asarray(x)) for x in B.conditioning(golden("g7_frame_coarse"), latents)]
    bg_all = (t(scene["bg"]).float() / 255.0).reshape(-1, 3).to(dev)
    tgt, m = torch.rand(N, 3, generator=torch.Generator().manual_seed(5)), R.matte(N)
    loss_fn = lambda rh, rc, s: R.colour_loss(rh, rc, tgt) + R.stats_loss(s, m)
    frame = engine.make_frame(H, W, scene["focal"], scene["cx"], scene["cy"], scene["poses"][B.FRAME], scene["pose_body"], orc.near, orc.far,
                              1e10, 0, N, 64, n_fine, 2, True)
    args = (orc.state, scene, zs, za, (sig_h.reshape(1, 96), sig_t), "f32", 64, n_fine, N)
    got = _step(*args, frame=frame, bg=bg_all, loss_fn=loss_fn, pix=pix)
    z = got["z"] if n_fine else O.coarse_z(orc.near, orc.far, 64)[None].expand(N, 64)
    if n_fine:
        assert bool((z[:, 1:] >= z[:, :-1]).all()) and float((z[:, -1] - orc.far).abs().max()) == 0.0
    ref = _oracle_step(orc, z, tgt, m, torch.float32)
    ref64 = None
    np.testing.assert_allclose(got["loss"], ref[0], rtol=3e-5)
    e_st = (got["stats"] - ref[5]).abs().max(0).values
    print(f"stats step, f32, 64+{n_fine}: loss {got['loss']:.6f} (oracle {ref[0]:.6f}); max |stats - oracle| {e_st.tolist()}")
    assert bool(torch.isfinite(got["stats"]).all())          # (the stats' own gate is the kernel test's; here they enter the loss)
    worst, worst_dir, worst_cos, n_seen = 0.0, 0.0, 1.0, 0
    for k, g in got["grads"].items():
        r = ref[1].get(k)
        rn = 0.0 if r is None else float(r.double().norm())
        if rn == 0.0:
            assert g is None or float(g.abs().max()) <= 1e-12, k
            continue
        gn = float(g.double().norm())
        e_n, d = abs(gn - rn) / rn, float((g - r).double().norm()) / rn
        cos = float(g.double().reshape(-1) @ r.double().reshape(-1)) / (gn * rn)
        if k in F64_YARDSTICK and not (e_n <= 1e-3 and d <= 5e-4 and cos >= 1 - 1e-6):
            ref64 = ref64 or _oracle_step(orc, z, tgt, m, torch.float64)
            own = rel_err(r, ref64[1][k])
            print(f"    {k}: {d:.2e} from the f32 oracle; {rel_err(g, ref64[1][k]):.2e} from float64, the f32 oracle's own {own:.2e}")
            assert rel_err(g, ref64[1][k]) <= 4 * own, k
            continue
        worst, worst_dir, worst_cos, n_seen = max(worst, e_n), max(worst_dir, d), min(worst_cos, cos), n_seen + 1
        assert e_n <= 1e-3, (k, gn, rn)
        assert cos >= 1.0 - 1e-6, (k, cos)
        assert d <= 5e-4, (k, d)
    e_sh, e_st_ = rel_err(got["d_sh"], ref[2]), rel_err(got["d_st"], ref[3])
    print(f"    worst relative gradient-norm error {worst:.2e}, worst whole-tensor error {worst_dir:.2e}, worst cosine {worst_cos:.8f} over "
          f"{n_seen} tensors; d sig_head {e_sh:.2e}, d sig_torso {e_st_:.2e}")
    assert n_seen > 40 and any(k.startswith(B.TORSO_ONLY) for k in got["grads"])
    assert e_sh < 2e-3 and e_st_ < 2e-3
    # the same step on pinhole rays that require grad: rays.grad against the oracle with the four ray blocks as leaves, everything else
    # torch.equal to the step on the detached rays
    bg = bg_all[pix.to(dev)].contiguous()
    rays0 = training.pinhole_rays(scene["poses"][B.FRAME], scene["pose_body"], pix.to(dev), H, W, scene["focal"], scene["cx"], scene["cy"])
    fr = _rays_frame(N, 64, n_fine, near=orc.near, far=orc.far)
    plain = _step(*args, frame=fr, bg=bg, loss_fn=loss_fn, rays=rays0.detach())
    rg = rays0.detach().clone().requires_grad_(True)
    grad = _step(*args, frame=fr, bg=bg, loss_fn=loss_fn, rays=rg)
    _assert_same_step(plain, grad, "rays.requires_grad with a stats loss", n_fine > 0)
    assert torch.equal(plain["stats"], grad["stats"]) and rg.grad is not None
    zr = grad["z"] if n_fine else z
    blocks = [rays0.detach().cpu()[:, 3 * k:3 * k + 3].contiguous() for k in range(4)]
    ref_r = _oracle_step(orc, zr, tgt, m, torch.float32, rays=blocks)[4]
    e_r = rel_err(rg.grad, ref_r)
    print(f"    rays.grad with the stats loss: {e_r:.2e} from the f32 oracle (max |ref| {float(ref_r.abs().max()):.2e})")
    assert float(ref_r.abs().max()) > 0 and bool(torch.isfinite(rg.grad).all())
    assert e_r < 2e-3


# ---- 4. the bf16 tier -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fine", [0, 128])
def test_bf16_tier_stats_on_its_own_samples_and_a_short_fit(orc, scene, latents, golden, n_fine):
    """what the stats add to the 16-bit tier is f32 code on f32 samples: stats and dsamples of the kernels on the samples, depths and
    ranks a bf16 step recorded against integrate_fields and its autograd on those samples, at the f32 tolerances of the kernel test;
    ten Adam steps on a fixed batch with the stats loss alone lower it, and two runs of them agree bit for bit"""
    from dfanerf import engine
    from dfanerf._lib import check, lib
    dev = torch.device("cuda")
    pix = t(orc.pix).long()
    H, W, S = scene["H"], scene["W"], 64 + n_fine
    sig_h, sig_t, zs, za = [t(np.asarray(x)) for x in B.conditioning(golden("g7_frame_coarse"), latents)]
    bg_all = (t(scene["bg"]).float() / 255.0).reshape(-1, 3).to(dev)
    m = R.matte(N)
    loss_fn = lambda rh, rc, s: R.stats_loss(s, m)
    frame = engine.make_frame(H, W, scene["focal"], scene["cx"], scene["cy"], scene["poses"][B.FRAME], scene["pose_body"], orc.near, orc.far,
                              1e10, 0, N, 64, n_fine, 2, True)
    args = (orc.state, scene, zs, za, (sig_h.reshape(1, 96), sig_t), "bf16", 64, n_fine, N)
    one = _step(*args, frame=frame, bg=bg_all, loss_fn=loss_fn, pix=pix)
    buf = one["buf"]
    sm = one["samples"].reshape(N, S, 8)
    assert bool(torch.isfinite(sm).all())
    if n_fine:
        z = one["z"]
        idx = one["ranks"].long()
        inv = torch.empty_like(idx)
        inv.scatter_(1, idx, torch.arange(S)[None].expand(N, S))
        order = lambda x: torch.gather(x, 1, inv[..., None].expand(N, S, 8))
    else:
        z, order = O.coarse_z(orc.near, orc.far, 64)[None].expand(N, 64).contiguous(), (lambda x: x)
    leaf = sm.clone().requires_grad_(True)
    mg = order(leaf)
    _, wh, _, wc = O.integrate_fields(z, orc.rays[1], orc.rays[3], mg[..., 0], mg[..., 1:4], mg[..., 4], mg[..., 5:8], orc.bg)
    ref = R.stats_of(wh, wc, z)
    e = (one["stats"] - ref.detach()).abs().max(0).values
    print(f"bf16 step, 64+{n_fine}: max |stats - integrate_fields on the recorded samples| {e.tolist()}")
    assert float(e[[0, 2]].max()) <= S * 2e-6 and float(e[[1, 3]].max()) <= orc.far * S * 2e-6
    d_s = torch.randn(N, 4, generator=torch.Generator().manual_seed(3))
    (ref * d_s).sum().backward()
    ds = torch.full((N, S, 8), float("nan"), device=dev)
    zero3, DS, PIX = torch.zeros(N, 3, device=dev), d_s.to(dev), pix.to(dev, torch.int32)
    check(lib.dfn_composite_bwd_stats(C.byref(frame), _p(PIX), None, None, _p(bg_all), None, _p(buf.samples), _p(buf.z_all), _p(buf.ranks),
                                      _p(zero3), _p(zero3), _p(DS), _p(ds), None, 0, None, _st()), "dfn_composite_bwd_stats")
    torch.cuda.synchronize()
    got_ds, ref_ds = ds.cpu().numpy(), leaf.grad.numpy()
    print(f"    max |d samples - autograd| {np.abs(got_ds - ref_ds).max():.2e} (max |ref| {np.abs(ref_ds).max():.2e})")
    assert np.abs(ref_ds).max() > 0
    np.testing.assert_allclose(got_ds, ref_ds, atol=2e-5 * np.abs(ref_ds).max(), rtol=2e-4)
    # ten Adam steps on the stats loss alone
    # (lr: the oracle's own autograd + torch Adam on this batch, coarse, goes 0.379 -> 0.216 monotonically at 5e-6; at the scripts'
    # 5e-4 its first step throws every composite opaque, 0.379 -> 0.713, and stays there - the blend decoder's density bias is delicate)
    a = _step(*args, frame=frame, bg=bg_all, loss_fn=loss_fn, pix=pix, steps=10, lr=5e-6)
    b = _step(*args, frame=frame, bg=bg_all, loss_fn=loss_fn, pix=pix, steps=10, lr=5e-6)
    print(f"    stats loss over ten Adam steps: {a['losses'][0]:.5f} -> {a['losses'][-1]:.5f}")
    assert np.isfinite(a["losses"]).all() and a["losses"][-1] < a["losses"][0]
    assert a["losses"] == b["losses"] and all(torch.equal(a["params"][k], b["params"][k]) for k in a["params"])
    assert a["losses"][0] == one["loss"]
