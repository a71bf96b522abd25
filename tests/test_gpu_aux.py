"""Opacity and expected depth from the fused renderer (dfn_render_fwd_aux / dfn_render_fwd_u8_aux; csrc/dfn_render_*_aux.hip) on the
GPU.  Per ray and image: acc = sum over FG of w_i, depth = sum over FG of w_i * z_i (premultiplied), FG = every sample of the final
pass but the background plane (include/dfanerf.h).

  1. the aux kernels return the plain kernels' RGB bit for bit;
  2. acc / depth against the same tier's own weights and depths (the plain call's want_weights / want_z), reduced in float64:
     |acc - acc64| <= S 2^-23, |depth - depth64| <= z_far S 2^-23 (at most S f32 roundings of partial sums <= 1, doubled);
  3. the exact tier against the CPU oracle: S * 2e-6 and z_far * S * 2e-6 (the project's per-weight gate, summed);
  4. the rays of 3. hold transparent and opaque ones.  THE SYNTHETIC SCENE'S COMPOSITE IMAGE IS OPAQUE EVERYWHERE (oracle, every
     101st pixel of frames 0 / 2 / 5 and six torso signals: acc_com >= 0.99999; its sigma_out.bias is -27 and the torso's raw sigma
     runs to several hundred), so 3. and 4. run on two decoders: the fixtures' (head image: 0.09 ... 0.99997) and the same network
     with sigma_out.bias lowered by 80, whose COMPOSITE image has both classes (oracle, the 131 rays used: 6 ... 15 below 0.1 and
     70 ... 86 above 0.5 at 64, 32, 128 and 64 + 128 samples);
  5. the u8 route equals the documented formulas applied to the f32 aux, exactly;
  6. refusals; 7. the CLI's --save_alpha / --save_depth files."""
import os

import numpy as np
import pytest
import torch

import dfa_oracle as O
from dfanerf import synth
from test_gpu_driver import COMMON, F_VAL, H, W, _run, dataset      # noqa: F401  (its synthetic dataset on disk, as a fixture of this module too)

pytestmark = pytest.mark.gpu

TIERS = ("f32", "f16", "f16x3")
FRAME = 2
SIGMA_SHIFT = -80.0


def t(x):
    return torch.from_numpy(np.asarray(x))


@pytest.fixture(scope="module")
def eng():
    from dfanerf import engine
    engine.require_gpu()
    return engine


@pytest.fixture(scope="module")
def packed(eng, states):
    flat = eng.flatten_state(states["decoder"], "cuda")
    return {tier: eng.PackedDecoder(flat, tier) for tier in TIERS}


@pytest.fixture(scope="module")
def narrow(eng, golden):
    """a decoder of hidden width 128 on the native 128-wide program, as tests/test_gpu_narrow.py builds it"""
    flat = eng.flatten_state(synth.synth_decoder_state(0, z_dim=64, hidden=128), "cuda")
    g3 = golden("g3_decoder")
    zs, za = synth.synth_latents(0, z_dim=64)
    return ({tier: eng.PackedDecoder(flat, tier, z_dim=64, width=128) for tier in TIERS},
            (g3["sig_aud"][0], g3["sig_torso"][0], zs[0], za[0]))


@pytest.fixture(scope="module")
def cond(golden, latents):
    g = golden("g7_frame_coarse")
    return g["signal"][0], g["signal_torso"].reshape(-1), latents[0][0], latents[1][0]


@pytest.fixture(scope="module")
def rays(golden):
    return golden("g7_frame_coarse")["ray_idx"][::8].astype(np.int32)          # 261 rays: a ragged last workgroup (8 / 4 rays each)


def _frame(eng, scene, n, n_coarse=64, n_fine=0, fields=2, cbg=True, begin=0):
    return eng.make_frame(scene["H"], scene["W"], scene["focal"], scene["cx"], scene["cy"], scene["poses"][FRAME], scene["pose_body"],
                          scene["near"], scene["far"], ray_begin=begin, ray_count=n, n_coarse=n_coarse, n_fine=n_fine, fields=fields,
                          concate_bg=cbg)


def _bg(scene):
    return (t(scene["bg"]).float() / 255.0).reshape(-1, 3).cuda()


def _plain_and_aux(eng, pk, cnd, scene, pix, **kw):
    """the same rays through dfn_render_fwd (with its weights and depths) and dfn_render_fwd_aux -> numpy"""
    sa, stt, zs, za = cnd
    fields = kw.get("fields", 2)
    n = kw.pop("n", None) if pix is None else len(pix)
    bias = pk.fold(sa, stt if fields == 2 else None, zs, za)
    fr = _frame(eng, scene, n, **kw)
    bg = _bg(scene)
    px = None if pix is None else t(pix).cuda()
    plain = eng.render(pk, bias, fr, bg, pix_index=px, want_weights=True, want_z=True)
    aux = eng.render(pk, bias, fr, bg, pix_index=px, want_aux=True)
    torch.cuda.synchronize()
    cpu = lambda o: None if o is None else o.cpu().numpy()
    return [cpu(o) for o in plain], [cpu(o) for o in aux]


def _check(plain, aux, S, fields, cbg, z_far, what):
    rh, rc, wh, wc, z = plain
    ah_rgb, ac_rgb, ah, ac = aux
    # 1. the RGB is the plain kernel's, bit for bit
    assert np.array_equal(ah_rgb, rh), what
    assert (rc is None and ac_rgb is None and ac is None) if fields == 1 else np.array_equal(ac_rgb, rc), what
    assert np.isfinite(rh).all() and float(rh.std()) > 0.01, what
    # 2. acc / depth against the kernel's own weights, reduced in float64
    assert z.shape[1] == S and wh.shape[1] == S
    n_fg = S - 1 if cbg else S
    worst = []
    for a, w in ((ah, wh), (ac, wc)):
        if a is None:
            continue
        assert a.shape == (len(rh), 2) and a.dtype == np.float32
        w64, z64 = w[:, :n_fg].astype(np.float64), z[:, :n_fg].astype(np.float64)
        e_acc = np.abs(a[:, 0] - w64.sum(1)).max()
        e_dep = np.abs(a[:, 1] - (w64 * z64).sum(1)).max()
        worst.append((e_acc, e_dep))
        assert e_acc <= S * 2.0 ** -23, (what, e_acc)
        assert e_dep <= z_far * S * 2.0 ** -23, (what, e_dep)
        assert (a[:, 0] >= 0).all() and (a[:, 0] <= 1 + S * 2.0 ** -23).all() and (a[:, 1] <= a[:, 0] * z_far + z_far * S * 2.0 ** -23).all()
        if not cbg:
            assert np.abs(a[:, 0] - w.astype(np.float64).sum(1)).max() <= 1e-5, what
            np.testing.assert_allclose(a[:, 0], 1.0, atol=1e-5)          # (test_render_coarse_f32_vs_reference_golden's gate on wh.sum(1))
    return worst


@pytest.mark.parametrize("tier", TIERS)
def test_rgb_unchanged_and_aux_matches_the_kernels_own_weights(eng, packed, narrow, cond, scene, rays, tier):
    pk = packed[tier]
    z_far = float(np.float32(scene["far"]))
    worst = []
    for fields in (1, 2):
        for n_fine in (0, 128):
            for cbg in (True, False):
                plain, aux = _plain_and_aux(eng, pk, cond, scene, rays, n_fine=n_fine, fields=fields, cbg=cbg)
                worst += _check(plain, aux, 64 + n_fine, fields, cbg, z_far, (tier, fields, n_fine, cbg))
    for n_coarse in (32, 128):                                 # the other coarse sample counts (no fine pass)
        plain, aux = _plain_and_aux(eng, pk, cond, scene, rays, n_coarse=n_coarse)
        worst += _check(plain, aux, n_coarse, 2, True, z_far, (tier, "n_coarse", n_coarse))
    # a contiguous ray range (no pix_index) that is no multiple of the workgroup's rays, in the middle of the frame
    begin = (scene["H"] // 2) * scene["W"] + 17
    for n_fine in (0, 128):
        plain, aux = _plain_and_aux(eng, pk, cond, scene, None, n=61, n_fine=n_fine, begin=begin)
        worst += _check(plain, aux, 64 + n_fine, 2, True, z_far, (tier, "61 rays", n_fine))
    # hidden width 128 through the native 128-wide program
    npk, ncond = narrow
    assert npk[tier].width == 128
    for fields, n_fine, cbg in ((2, 128, True), (1, 0, False), (2, 0, True)):
        plain, aux = _plain_and_aux(eng, npk[tier], ncond, scene, rays, n_fine=n_fine, fields=fields, cbg=cbg)
        worst += _check(plain, aux, 64 + n_fine, fields, cbg, z_far, (tier, "width 128", fields, n_fine, cbg))
    print(f"{tier}: max |acc - acc64| {max(w[0] for w in worst):.2e}, max |depth - depth64| {max(w[1] for w in worst):.2e} "
          f"(bounds at S = 64: {64 * 2.0 ** -23:.2e}, {z_far * 64 * 2.0 ** -23:.2e})")


# ---- 3. / 4. the exact tier against the oracle ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_cases(eng, states, latents, scene, golden):
    """both decoders (module docstring, 4.), rays of golden G7 / 16: per case the GPU's aux and the oracle's weights and depths.
    Coarse only at 64, 32 and 128 samples: O.render_rays_chunk(return_aux=True); 64 + 128: the oracle's fields at the depths the GPU's
    plain call returns (O._eval_fields + O.integrate_fields, as O.render_fixed_samples does)."""
    g = golden("g7_frame_coarse")
    idx = g["ray_idx"][::16].astype(np.int32)
    zs, za = latents
    bg = (t(scene["bg"]).float() / 255.0).reshape(-1, 3)
    geo = (scene["H"], scene["W"], scene["focal"])
    o_h, d_h = O.get_rays(*geo, scene["poses"][FRAME][:3, :4], scene["cx"], scene["cy"])
    o_t, d_t = O.get_rays(*geo, scene["pose_body"][:3, :4], scene["cx"], scene["cy"])
    r = [x.reshape(-1, 3)[idx] for x in (o_h, d_h, o_t, d_t)]
    sig, sigt = [t(g["signal"]), None], t(g["signal_torso"]).reshape(1, -1)
    cnd = (g["signal"][0], g["signal_torso"].reshape(-1), zs[0], za[0])
    cases = []
    for name, shift in (("fixture decoder", 0.0), ("sigma_out.bias - 80", SIGMA_SHIFT)):
        st = dict(states["decoder"])
        st["sigma_out.bias"] = (st["sigma_out.bias"] + np.float32(shift)).astype(np.float32)
        P = O.params_to_torch(st)
        pk = eng.PackedDecoder(eng.flatten_state(st, "cuda"), "f32")
        for S, n_fine in ((64, 0), (32, 0), (128, 0), (64, 128)):
            plain, aux = _plain_and_aux(eng, pk, cnd, scene, idx, n_coarse=S, n_fine=n_fine)
            with torch.no_grad():
                if n_fine == 0:
                    _, _, oa = O.render_rays_chunk(P, *r, bg[idx], scene["near"], scene["far"], t(zs), t(za), sig, sigt, S, 0, 2,
                                                   return_aux=True)
                    w_h, w_c, z = oa["w_head"], oa["w_com"], oa["z_coarse"]
                else:
                    z = t(plain[4])
                    s_h, f_h, s_t, f_t = O._eval_fields(P, *r, z, t(zs), t(za), sig, sigt, 2)
                    _, w_h, _, w_c = O.integrate_fields(z, r[1], r[3], s_h, f_h, s_t, f_t, bg[idx])
            cases.append({"name": f"{name}, {S} + {n_fine}", "shifted": shift != 0.0, "S": S + n_fine, "aux_head": aux[2], "aux_com": aux[3],
                          "w_head": w_h.double().numpy(), "w_com": w_c.double().numpy(), "z": z.double().numpy()})
    return cases


def _oracle_acc_depth(c, img):
    w, z = c["w_" + img][:, :-1], c["z"][:, :-1]                # concate_bg: FG = every sample but the last
    return w.sum(1), (w * z).sum(1)


def test_oracle_rays_are_not_vacuous(oracle_cases, scene):
    for c in oracle_cases:
        acc, dep = _oracle_acc_depth(c, "com" if c["shifted"] else "head")
        # the composite image of the decoder with the lowered sigma bias (the fixtures' composite is opaque everywhere: there the
        # head image, which the issue does not ask for, is held to the opaque half and the depth range)
        if c["shifted"]:
            assert (acc < 0.1).any() and (acc > 0.5).any(), (c["name"], float(acc.min()), float(acc.max()))
        opaque = acc > 0.5
        assert opaque.any(), c["name"]
        mean_depth = dep[opaque] / acc[opaque]
        assert (mean_depth > scene["near"]).all() and (mean_depth < scene["far"]).all(), (c["name"], mean_depth.min(), mean_depth.max())
    acc_c, _ = _oracle_acc_depth(oracle_cases[0], "com")
    assert acc_c.min() > 0.999                                   # what the module docstring says about the fixtures' composite


def test_aux_against_the_oracle_exact_tier(oracle_cases, scene):
    z_far = float(scene["far"])
    for c in oracle_cases:
        S = c["S"]
        for img in ("head", "com"):
            acc, dep = _oracle_acc_depth(c, img)
            a = c["aux_" + img]
            e_acc, e_dep = np.abs(a[:, 0] - acc).max(), np.abs(a[:, 1] - dep).max()
            print(f"{c['name']}, {img}: max |acc - oracle| {e_acc:.2e} (gate {S * 2e-6:.1e}), max |depth - oracle| {e_dep:.2e} "
                  f"(gate {z_far * S * 2e-6:.1e}); acc in [{acc.min():.4f}, {acc.max():.4f}]")
            assert e_acc <= S * 2e-6, (c["name"], img, e_acc)
            assert e_dep <= z_far * S * 2e-6, (c["name"], img, e_dep)


# ---- 5. the u8 route -----------------------------------------------------------------------------------------------------------
def _to_alpha8(acc):
    return (np.float32(255.0) * np.clip(acc.astype(np.float32), np.float32(0), np.float32(1))).astype(np.int32).astype(np.uint8)


def _to_depth16(dep, z_far):
    q = np.clip(dep.astype(np.float32) / np.float32(z_far), np.float32(0), np.float32(1))
    return (np.float32(65535.0) * q).astype(np.int32).astype(np.uint16)


@pytest.mark.parametrize("tier", TIERS)
def test_u8_route_is_the_documented_formulas_on_the_f32_aux(eng, packed, cond, scene, rays, tier):
    pk = packed[tier]
    sa, stt, zs, za = cond
    bg, px = _bg(scene), t(rays).cuda()
    cpu = lambda o: None if o is None else o.cpu().numpy()
    for fields, n_fine in ((2, 128), (2, 0), (1, 0)):
        bias = pk.fold(sa, stt if fields == 2 else None, zs, za)
        fr = _frame(eng, scene, len(rays), n_fine=n_fine, fields=fields)
        _, _, ah, ac = [cpu(o) for o in eng.render(pk, bias, fr, bg, pix_index=px, want_aux=True)]
        p_h, p_c = [cpu(o) for o in eng.render_u8(pk, bias, fr, bg, pix_index=px)]
        full = [cpu(o) for o in eng.render_u8(pk, bias, fr, bg, pix_index=px, want_alpha=True, want_depth=True)]
        only_a = [cpu(o) for o in eng.render_u8(pk, bias, fr, bg, pix_index=px, want_alpha=True)]           # the depth pair NULL
        only_d = [cpu(o) for o in eng.render_u8(pk, bias, fr, bg, pix_index=px, want_depth=True)]           # the alpha pair NULL
        torch.cuda.synchronize()
        assert len(full) == 6 and len(only_a) == 4 and len(only_d) == 4
        for out in (full, only_a, only_d):
            assert np.array_equal(out[0], p_h) and (np.array_equal(out[1], p_c) if fields == 2 else out[1] is None)
        want = {"a_h": _to_alpha8(ah[:, 0]), "d_h": _to_depth16(ah[:, 1], fr.z_far)}
        got = {"a_h": (full[2], only_a[2]), "d_h": (full[4], only_d[2])}
        if fields == 2:
            want.update({"a_c": _to_alpha8(ac[:, 0]), "d_c": _to_depth16(ac[:, 1], fr.z_far)})
            got.update({"a_c": (full[3], only_a[3]), "d_c": (full[5], only_d[3])})
        else:
            assert full[3] is None and full[5] is None
        for k, w in want.items():
            for g_ in got[k]:
                assert g_.dtype == w.dtype and g_.shape == (len(rays),) and np.array_equal(g_, w), (tier, fields, n_fine, k)
        assert want["a_h"].min() < want["a_h"].max() and want["a_h"].max() > 250 and want["d_h"].max() > 10000      # a matte, not a constant


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(eng, states, packed, cond, scene, rays):
    import ctypes as C
    from dfanerf import _lib
    sa, stt, zs, za = cond
    bg, px = _bg(scene), t(rays).cuda()
    fr = _frame(eng, scene, len(rays))
    sentinel = lambda: torch.full((len(rays), 3), -7.0, device="cuda")
    # the bf16 tier (the training tier) has no aux kernels
    pk16 = eng.PackedDecoder(eng.flatten_state(states["decoder"], "cuda"), "bf16")
    oh, oc = sentinel(), sentinel()
    with pytest.raises(_lib.DfnError, match="bf16"):
        eng.render(pk16, pk16.fold(sa, stt, zs, za), fr, bg, pix_index=px, want_aux=True, out_head=oh, out_com=oc)
    with pytest.raises(_lib.DfnError, match="bf16"):
        eng.render_u8(pk16, pk16.fold(sa, stt, zs, za), fr, bg, pix_index=px, want_alpha=True)
    # a NULL aux_head
    pk = packed["f32"]
    bias = pk.fold(sa, stt, zs, za)
    p = lambda x: C.c_void_p(x.data_ptr())
    aux_c = torch.full((len(rays), 2), -7.0, device="cuda")
    rc = _lib.lib.dfn_render_fwd_aux(pk.tier_arg, C.byref(fr), p(pk.packed[0]), p(pk.packed[1]), p(bias),
                                     C.c_void_p(bias.data_ptr() + 4 * pk.bias_floats(0)), p(bg), None, p(px), p(oh), p(oc), None, p(aux_c), None)
    assert rc == -1 and b"aux_head" in _lib.lib.dfn_last_error()
    # want_aux together with the per-sample outputs
    with pytest.raises(ValueError, match="want_aux"):
        eng.render(pk, bias, fr, bg, pix_index=px, want_aux=True, want_weights=True, out_head=oh, out_com=oc)
    with pytest.raises(ValueError, match="want_aux"):
        eng.render(pk, bias, fr, bg, pix_index=px, want_aux=True, want_z=True, out_head=oh, out_com=oc)
    torch.cuda.synchronize()
    assert bool((oh == -7.0).all()) and bool((oc == -7.0).all()) and bool((aux_c == -7.0).all())        # nothing ran


# ---- 7. the CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_save_alpha_save_depth(dataset, monkeypatch):
    """tests/test_gpu_driver.py's --render_person run (its dataset fixture and flag bundle) with --save_alpha --save_depth --hip_tier
    f16, in a fresh child process: the planes next to every frame, their modes and size, equal to engine.render_u8's for one frame,
    and the RGB files equal to a run without the flags"""
    from PIL import Image
    from dfanerf import engine, run_nerf
    from dfanerf.load_audface import load_audface_data_split
    root, sc = dataset
    base = "--render_person --test_file transforms_val_ba.json --N_rand=2048 --N_iters=600000 --image_ext png --hip_tier f16"
    out = root / "dataset" / "train_together" / "obama_TrainExpLater_smoMix" / "obama" / "person"
    _run(root, base)
    plain = {sub: {f: (out / sub / f).read_bytes() for f in sorted(os.listdir(out / sub))} for sub in ("render_com", "render_head")}
    assert sorted(plain["render_com"]) == [f"test_{i:06d}.png" for i in range(F_VAL)]
    _run(root, base + " --save_alpha --save_depth")
    for sub in ("render_com", "render_head"):
        names = sorted(os.listdir(out / sub))
        assert names == sorted(f"test_{i:06d}{s}.png" for i in range(F_VAL) for s in ("", "_alpha", "_depth")), names
        for f, blob in plain[sub].items():
            assert (out / sub / f).read_bytes() == blob, (sub, f)                         # the RGB files: byte for byte
        for i in range(F_VAL):
            a, d = Image.open(out / sub / f"test_{i:06d}_alpha.png"), Image.open(out / sub / f"test_{i:06d}_depth.png")
            assert a.mode == "L" and d.mode == "I;16" and a.size == (W, H) and d.size == (W, H), (a.mode, d.mode, a.size)
    # frame 1 through the library in this process: the CLI's checkpoint, dataset, signal encoders and frame renderer
    k = 1
    monkeypatch.chdir(root)
    args = run_nerf.config_parser().parse_args((COMMON + " " + base + " --save_alpha --save_depth").split())
    dev = torch.device("cuda")
    nets, opts, _ = run_nerf.create_nerf(args, dev)
    step, z_shape, z_app = run_nerf.load_checkpoint(args.resume, nets, opts, map_location=dev)
    ds = load_audface_data_split(args.datadir, args.testskip, test_file=args.test_file, aud_file=args.aud_file, exp_file=args.exp_file,
                                 use_ba=True)
    R = run_nerf.FrameRenderer(nets["decoder"], z_shape.to(dev), z_app.to(dev), t(ds["bc_img"]).to(dev).float() / 255.0, ds["hwfcxy"],
                               args.near, args.far, args)
    assert R.tier == "f16" and R.save_alpha and R.save_depth
    dd = {kk: t(ds[kk]).to(dev).float() for kk in ("auds", "exp", "poses")}
    enc = engine.SignalEncoder(nets["AudNet"], nets["ExpNet"], nets["AudAttNet"], nets["PoseAttNet"], dd["auds"], dd["exp"], dd["poses"])
    smo = step >= args.nosmo_iters
    s2, t2 = enc.encode([k], args.smo_size if smo else 0, args.smo_torse_size if smo else 0, length=F_VAL)
    pk = R.decoder.packed(R.tier)
    bias = pk.fold(s2[0], t2[0], R.zs, R.za)
    res = R.render(ds["poses"][k][:3, :4], np.asarray(sc["poses"][0], np.float32)[:3, :4], None, None, out_u8=True, bias=bias,
                   want_alpha=True, want_depth=True)
    torch.cuda.synchronize()
    rh, rc, a_h, a_c, d_h, d_c = [o.cpu().numpy() for o in res]
    for sub, rgb, a8, d16 in (("render_com", rc, a_c, d_c), ("render_head", rh, a_h, d_h)):
        assert np.array_equal(np.asarray(Image.open(out / sub / f"test_{k:06d}.png").convert("RGB")), rgb.reshape(H, W, 3)), sub
        got_a = np.asarray(Image.open(out / sub / f"test_{k:06d}_alpha.png"))
        got_d = np.asarray(Image.open(out / sub / f"test_{k:06d}_depth.png")).astype(np.uint16)
        assert got_a.dtype == np.uint8 and np.array_equal(got_a, a8.reshape(H, W)), sub
        assert np.array_equal(got_d, d16.reshape(H, W)), sub
    assert a_h.min() < 128 < a_h.max() or a_c.max() > 250                                # a matte, not an empty plane
