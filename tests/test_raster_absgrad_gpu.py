"""AbsGS' absolute screen-space gradient on the HIP path (`rasterize_backward(abs_grad_out=)` = syn3r_raster_backward_abs, the ABS
instances of the blend backward) against the float64 reference of tests/raster_absgrad_ref.py: the four scenes with and without a
depth gradient, the anti-aliased, filtered and raw-parameter modes, "the signed outputs do not move", |signed| <= abs, the statistics
entry syn3r_densification_stats_abs, and the trainer (both step routes, AbsGS' split rule, "off is the old call path").  Every test
needs the new entries."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_aa_ref as A  # noqa: E402
import raster_absgrad_ref as R  # noqa: E402
import raster_f3d_ref as F  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 2e-3          # the project's bar for rasteriser gradients (tests/test_raster_gpu.py, tests/test_raster_aa_gpu.py)


def settings(sc, dev, deg, aa=False):
    from syn3r_amd.raster import GaussianRasterizationSettings
    f = lambda t: t.float().to(dev)
    return GaussianRasterizationSettings(sc["H"], sc["W"], sc["tfx"], sc["tfy"], f(sc["bg"]), 1.0, f(sc["view"]), f(sc["proj"]), deg,
                                         f(sc["campos"]), False, False, aa)


def hip_backward(sc, dev, deg, weights, depth_grad=True, aa=False, filt=None, with_abs=True):
    """-> (radii, the 7-tuple of rasterize_backward, abs [N,2] or None): activated tensors in, the weights as upstream gradients
    (the loss is linear in the outputs); no dL_ddepth without `depth_grad`.  The buffer is handed over full of NaN: every row has
    to be written."""
    from syn3r_amd.raster import rasterize_backward, rasterize_forward
    f = lambda t: t.to(dev, torch.float32).contiguous()
    cf = f(sc["cf"]) if sc["cf"] is not None else None
    wc, wd, wa = (f(w) for w in weights)
    with torch.no_grad():
        _, radii, _, _, st = rasterize_forward(f(sc["m"]), f(sc["sh"]), f(sc["o"]), f(sc["s"]), f(sc["q"]), cf, settings(sc, dev, deg, aa),
                                               filter_3D=f(filt) if filt is not None else None)
        buf = torch.full((sc["N"], 2), float("nan"), device=dev) if with_abs else None
        grads = rasterize_backward(st, wc, wd if depth_grad else None, wa, abs_grad_out=buf)
    return radii, grads, buf


def compare(got, radii, ref_abs, tag, measurements, **extra):
    """max |hip - ref| / max |ref| per component below the bar; culled rows exact zeros; all finite and >= 0"""
    got64 = got.cpu().double()
    assert got.shape == ref_abs.shape and got.dtype == torch.float32
    assert bool(torch.isfinite(got64).all()) and bool((got64 >= 0).all())
    culled = (radii <= 0).cpu()
    assert int(culled.sum()) > 0 or ref_abs.shape[0] == 1
    assert float(got64[culled].abs().sum()) == 0.0
    err = [float((got64[:, c] - ref_abs[:, c]).abs().max()) / float(ref_abs[:, c].abs().max()) for c in (0, 1)]
    print(tag, extra, f"max |hip - ref| / max |ref|: x {err[0]:.3e}  y {err[1]:.3e}")
    measurements("raster_absgrad", tag=tag, err_x=err[0], err_y=err[1], **extra)
    assert err[0] < BAR and err[1] < BAR, (tag, err)
    return err


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("depth_grad", [True, False], ids=["depth", "nodepth"])
@pytest.mark.parametrize("shape", R.SCENES, ids=R.SCENE_IDS)
def test_abs_gradient_vs_reference(shape, depth_grad, gpu, measurements):
    """Both HAS_DEPTH_GRAD instances of the ABS variant on the four scenes (33 x 50 is no tile multiple; two to four tile lists of
    each run over more than one staging round; the opaque scene stops early).  Measured on an MI355X (profiles/r13/raster_absgrad.txt):
    <= 2.5e-6 of the reference's largest entry on every scene and instance, so the project's 2e-3 stands."""
    ref = R.reference(shape, depth_grad)
    radii, _, got = hip_backward(ref["sc"], gpu, ref["deg"], ref["weights"], depth_grad)
    compare(got, radii, ref["abs"], "plain", measurements, shape=list(shape), depth_grad=depth_grad)
    visible = (radii > 0).cpu()
    assert int((visible != ref["valid"]).sum()) <= 0.01 * shape[0]      # (an fp32 radius may land on the other side of an integer)
    if shape == R.OPAQUE:                     # the early stop on the device too: the Gaussians behind saturated pixels get nothing
        nz = int(((got.abs().sum(1) > 0).cpu() & visible).sum())
        assert 0 < nz <= 0.6 * int(visible.sum())


# ---------------------------------------------------------------------------------------------------------------- 2
def test_antialiased_mode(gpu, measurements):
    """the blend opacity carries rho: the reference blends raster_aa_ref.rasterize's `pre`"""
    shape = A.SHAPES[1]
    N, H, W, conf, deg, scale = shape
    sc = A.scene(N, H, W, conf, scale)
    weights = R.weights_of(H, W)
    with torch.no_grad():
        (_, _, _, _, aux), _, rho, _ = A.rasterize(sc, deg, True)
    ref = R.from_aux(sc, aux, weights)
    plain = R.reference(shape)
    assert float((ref["abs"] - plain["abs"]).abs().max()) > 0.05 * float(plain["abs"].max())        # the mode matters
    radii, _, got = hip_backward(sc, gpu, deg, weights, aa=True)
    compare(got, radii, ref["abs"], "antialias", measurements, shape=list(shape))


@pytest.mark.parametrize("aa", [False, True], ids=["f3d", "f3d_antialias"])
def test_filtered_mode(aa, gpu, measurements):
    """... and coef: raster_f3d_ref.rasterize's `pre` (filtered scales, opacity x coef [x rho])"""
    shape = A.SHAPES[0]
    sc, deg = F.scene(shape), shape[4]
    weights = R.weights_of(sc["H"], sc["W"])
    with torch.no_grad():
        (_, _, _, _, aux), _ = F.rasterize(sc, deg, sc["f"], aa)
    ref = R.from_aux(sc, aux, weights)
    radii, _, got = hip_backward(sc, gpu, deg, weights, aa=aa, filt=sc["f"])
    compare(got, radii, ref["abs"], "filter3d" + ("+antialias" if aa else ""), measurements, shape=list(shape))
    _, _, got_off = hip_backward(sc, gpu, deg, weights, aa=aa)
    assert float((got - got_off).abs().max()) > 0.01 * float(got.max())                             # the filter matters


def test_raw_route_equals_activated_route(gpu, measurements):
    """raw = 1 (log-scales, unnormalised quaternions, logits in) gives the activated route's absolute gradient, to the noise of the
    blend backward's atomics: 2e-5 of its largest entry.  The activated tensors are syn3r_gaussian_activate's of the raw ones, as in
    tests/test_raster_aa_gpu.py, so the two forwards are the same bits."""
    from syn3r_amd import _lib as L
    from syn3r_amd.raster import rasterize_backward, rasterize_forward
    N, H, W, conf, deg, scale = A.SHAPES[0]
    sc = A.scene(N, H, W, True, scale)
    f = lambda t: t.float().to(gpu).contiguous()
    g = torch.Generator().manual_seed(17)
    m3, sh, cf = f(sc["m"]), f(sc["sh"]), f(sc["cf"])
    ls = f(torch.log(sc["s"]))
    rr = f(sc["q"] * (0.5 + 1.5 * torch.rand(N, 1, generator=g, dtype=torch.float64)))
    lg = f(torch.log(sc["o"] / (1.0 - sc["o"]))).reshape(N, 1)
    lib, stream = L.load(), L.stream_ptr(gpu)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=gpu)
    wc, wd, wa = (f(w) for w in R.weights_of(H, W))
    res = {}
    with torch.no_grad():
        s_act, r_act, o_act = new(N, 3), new(N, 4), new(N, 1)
        L.check(lib.syn3r_gaussian_activate(N, L.ptr(ls), L.ptr(rr), L.ptr(lg), L.ptr(s_act), L.ptr(r_act), L.ptr(o_act), stream),
                "gaussian_activate")
        for aa in (False, True):
            st = settings(sc, gpu, deg, aa)
            *out0, s0 = rasterize_forward(m3, sh, o_act, s_act, r_act, cf, st)
            *out1, s1 = rasterize_forward(m3, sh, lg, ls, rr, cf, st, raw_params=True)
            for a, b in zip(out0, out1):
                assert torch.equal(a, b)
            a0, a1 = torch.full((N, 2), float("nan"), device=gpu), torch.full((N, 2), float("nan"), device=gpu)
            rasterize_backward(s0, wc, wd, wa, abs_grad_out=a0)
            rasterize_backward(s1, wc, wd, wa, abs_grad_out=a1)
            top = float(a0.max())
            diff = float((a0 - a1).abs().max())
            print(f"antialiasing={aa}: max |raw - activated| = {diff:.3e} of {top:.3e}; bit-equal: {torch.equal(a0, a1)}")
            measurements("raster_absgrad_raw_route", antialiasing=aa, rel=diff / top, bit_equal=bool(torch.equal(a0, a1)))
            assert top > 0 and bool(torch.isfinite(a1).all())
            assert diff <= 2e-5 * top
            assert float(a1[out1[1] <= 0].abs().sum()) == 0.0
            res[aa] = a1
    assert float((res[True] - res[False]).abs().max()) > 0.05 * float(res[False].max())           # the raw route honours the flag


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("depth_grad", [True, False], ids=["depth", "nodepth"])
def test_signed_outputs_do_not_move(depth_grad, gpu, measurements):
    """The seven tensors of rasterize_backward with `abs_grad_out` against those without: 2e-5 of each tensor's largest entry, the
    bound tests/test_raster_aa_gpu.py uses between two routes of one backward (the float atomics' order differs from launch to
    launch); whether they are in fact the same bits is printed and recorded."""
    shape = A.SHAPES[2]
    ref = R.reference(shape, depth_grad)
    _, with_abs, _ = hip_backward(ref["sc"], gpu, ref["deg"], ref["weights"], depth_grad)
    _, without, none = hip_backward(ref["sc"], gpu, ref["deg"], ref["weights"], depth_grad, with_abs=False)
    assert none is None
    names = ("means3D", "means2D", "shs", "opacities", "scales", "rotations", "confidence")
    assert len(with_abs) == len(without) == 7
    equal = {}
    for name, a, b in zip(names, with_abs, without):
        assert a.shape == b.shape
        top = float(b.abs().max()) + 1e-20
        diff = float((a - b).abs().max())
        equal[name] = bool(torch.equal(a, b))
        assert diff <= 2e-5 * top, (name, diff, top)
    print("signed outputs with / without abs_grad_out, bit-equal:", equal)
    measurements("raster_absgrad_signed_outputs", depth_grad=depth_grad, **equal)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("shape", R.SCENES, ids=R.SCENE_IDS)
def test_signed_is_bounded_by_abs(shape, gpu):
    """component-wise |d_means2D[:, :2]| <= abs2D + 1e-5 of the largest entry"""
    ref = R.reference(shape)
    _, grads, got = hip_backward(ref["sc"], gpu, ref["deg"], ref["weights"])
    signed = grads[1][:, :2].abs()
    assert float(signed.max()) > 0
    assert bool((signed <= got + 1e-5 * float(got.max())).all()), float((signed - got).max())


def test_cancellation_on_the_device(gpu):
    """the symmetric single Gaussian of the CPU tier: the plain norm is below 1e-3 of the absolute norm, which matches the reference"""
    ref = R.cancel_reference()
    _, grads, got = hip_backward(ref["sc"], gpu, 0, ref["weights"], depth_grad=False)
    an, pn = float(got[0].norm()), float(grads[1][0, :2].norm())
    ref_an = float(ref["abs"][0].norm())
    print(f"cancellation scene on the device: abs norm {an:.6g} (reference {ref_an:.6g}), plain norm {pn:.3e}")
    assert abs(an - ref_an) < BAR * ref_an
    assert pn < 1e-3 * an


# ---------------------------------------------------------------------------------------------------------------- 5
def test_densification_stats_abs_vs_masked_torch(gpu):
    """syn3r_densification_stats_abs == boolean-mask torch, bit for bit (the norms as sqrt(x*x + y*y), the kernel's expression: three
    correctly rounded fp32 operations on either side); about half the radii are <= 0 and those rows are untouched."""
    from syn3r_amd import _lib as L
    g = torch.Generator().manual_seed(11)
    n = 1000
    radii = torch.randint(-20, 21, (n,), generator=g, dtype=torch.int32).to(gpu)
    vgrad = torch.randn(n, 3, generator=g).to(gpu)
    agrad = torch.rand(n, 2, generator=g).to(gpu) * 3.0
    accum, accum_abs = torch.rand(n, 1, generator=g).to(gpu), torch.rand(n, 1, generator=g).to(gpu)
    denom = torch.randint(0, 5, (n, 1), generator=g).float().to(gpu)
    maxr = (torch.rand(n, generator=g) * 30).to(gpu)
    vis = radii > 0
    assert 0.4 * n < int(vis.sum()) < 0.6 * n and int((radii == 0).sum()) > 0
    ea, eb, ed, em = accum.clone(), accum_abs.clone(), denom.clone(), maxr.clone()
    norm2 = lambda t: torch.sqrt(t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1])[:, None]
    ea[vis] += norm2(vgrad[vis])
    eb[vis] += norm2(agrad[vis])
    ed[vis] += 1
    em[vis] = torch.max(em[vis], radii[vis].to(em.dtype))
    L.check(L.load().syn3r_densification_stats_abs(n, L.ptr(radii), L.ptr(vgrad), L.ptr(agrad), L.ptr(accum), L.ptr(accum_abs),
                                                   L.ptr(denom), L.ptr(maxr), L.stream_ptr(gpu)), "densification_stats_abs")
    assert torch.equal(denom, ed) and torch.equal(maxr, em)
    assert torch.equal(accum, ea) and torch.equal(accum_abs, eb)
    assert float((accum_abs - eb)[~vis].abs().sum()) == 0.0
    lib = L.load()
    assert lib.syn3r_densification_stats_abs(n, L.ptr(radii), L.ptr(vgrad), None, L.ptr(accum), L.ptr(accum_abs), L.ptr(denom),
                                             L.ptr(maxr), L.stream_ptr(gpu)) == -1 and b"null" in lib.syn3r_last_error()


# ---------------------------------------------------------------------------------------------------------------- 6
def make_scene(N, H, W, seed, dev):
    """tests/test_trainer_gpu.py::make_scene"""
    from oracle import raster_oracle as RO
    from syn3r_amd.gs import GaussianModel
    m, s, q, o, sh = RO.synthetic_gaussians(N, seed=seed, log_scale_mean=np.log(0.08))
    logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
    gm = GaussianModel(m, torch.log(s), q, logit, sh, device=dev)
    fx = W / (2 * math.tan(math.radians(30)))
    K = np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], dtype=np.float32)
    return gm, K


def test_trainer_both_routes_return_the_abs_gradient(gpu):
    """`densify_abs_grad=True`: the explicit step and the autograd step return the same `viewspace_abs_grad` (2e-5 of its largest
    entry) and, with the density control on, both fill `xyz_gradient_accum_abs` (the explicit route through the statistics entry,
    the autograd route through the masked-indexing fallback); with the option off neither key nor accumulator exists."""
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    from syn3r_amd.gs.train_ops import photometric_loss
    N, H, W = 2000, 64, 96
    w2c = np.eye(4, dtype=np.float32)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(5))
    got, acc = {}, {}
    for explicit in (True, False):
        gm, K = make_scene(N, H, W, 13, gpu)
        cam = Camera.from_w2c(w2c, K, H, W, image=target, data_device=gpu, cam_confidence=0.7)
        tr = GSTrainer(gm, [cam], OptimizationParams(iterations=10, densify_abs_grad=True))
        if explicit:
            _, out = tr._explicit_step(cam)
            vs = out["viewspace_grad"]
        else:
            out = tr.render_view(cam)
            assert float(out["viewspace_abs_grad"].abs().sum()) == 0.0          # filled by the backward
            photometric_loss(out["render"], cam.original_image, 0.2, 0.7).backward()
            vs = out["viewspace_points"].grad
        a = out["viewspace_abs_grad"]
        assert a.shape == (N, 2) and a.dtype == torch.float32 and not a.requires_grad
        assert bool((vs[:, :2].abs() <= a + 1e-5 * float(a.max())).all())
        assert float(a[out["radii"] <= 0].abs().sum()) == 0.0 and float(a.max()) > 0
        got[explicit] = a.clone()
        tr.densify = True
        tr.train_step(cam, explicit=explicit)
        assert gm.xyz_gradient_accum_abs.shape == (N, 1)
        acc[explicit] = (gm.xyz_gradient_accum_abs.clone(), gm.xyz_gradient_accum.clone(), gm.denom.clone())
    top = float(got[False].max())
    assert float((got[True] - got[False]).abs().max()) <= 2e-5 * top
    (a_abs, a_acc, a_den), (b_abs, b_acc, b_den) = acc[True], acc[False]
    assert torch.equal(a_den, b_den) and float(a_den.sum()) > N // 2
    assert float(a_abs.max()) > 0 and float((a_abs - b_abs).abs().max()) <= 2e-5 * float(b_abs.max())
    assert float((a_abs - got[True].norm(dim=1, keepdim=True)).abs().max()) <= 2e-5 * float(a_abs.max())   # one step: the norm itself
    assert bool((a_abs >= a_acc - 1e-5 * float(a_abs.max())).all())
    # option off: nothing of it
    gm, K = make_scene(N, H, W, 13, gpu)
    cam = Camera.from_w2c(w2c, K, H, W, image=target, data_device=gpu, cam_confidence=0.7)
    tr = GSTrainer(gm, [cam], OptimizationParams(iterations=10))
    _, out = tr._explicit_step(cam)
    assert "viewspace_abs_grad" not in out and "viewspace_abs_grad" not in tr.render_view(cam)
    tr.densify = True
    tr.train_step(cam)
    assert getattr(gm, "xyz_gradient_accum_abs", None) is None


def test_split_decision_on_the_abs_statistic(gpu):
    """Statistics set by hand - plain gradient 0 everywhere, absolute accumulator above the threshold on 7 chosen large Gaussians:
    `densify_and_prune` splits exactly those 7 with the option on (AbsGS' rule) and nothing with it off."""
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    N, H, W = 500, 40, 56
    w2c = np.eye(4, dtype=np.float32)
    for on in (True, False):
        gm, K = make_scene(N, H, W, 21, gpu)
        cam = Camera.from_w2c(w2c, K, H, W, image=torch.rand(3, H, W), data_device=gpu)
        tr = GSTrainer(gm, [cam], OptimizationParams(iterations=10, densify_abs_grad=on))
        o, extent = tr.opt, tr.cameras_extent()
        large = (gm.get_scaling.max(dim=1).values > o.percent_dense * extent).nonzero().squeeze(1)
        small = (gm.get_scaling.max(dim=1).values <= o.percent_dense * extent).nonzero().squeeze(1)
        assert large.numel() >= 20
        chosen = large[torch.arange(7, device=gpu) * (large.numel() // 7)]
        gm.ensure_stats(True)
        gm.denom.fill_(1.0)
        gm.xyz_gradient_accum.zero_()
        gm.xyz_gradient_accum_abs.zero_()
        gm.xyz_gradient_accum_abs[chosen] = 2.0 * o.densify_abs_grad_threshold
        gm.xyz_gradient_accum_abs[large[1]] = 0.5 * o.densify_abs_grad_threshold         # below the threshold
        if small.numel():
            gm.xyz_gradient_accum_abs[small[0]] = 10.0                                   # above it, but small: no split (and no clone)
        assert int(large[1]) not in chosen.tolist()
        xyz0 = gm._xyz.detach().clone()
        counts = tr.densify_and_prune(o.densify_grad_threshold, 0.0, extent, None)
        if on:
            assert counts == (0, 7, 0)
            keep = torch.ones(N, dtype=torch.bool, device=gpu)
            keep[chosen] = False
            assert gm._xyz.shape[0] == N - 7 + 14
            assert torch.equal(gm._xyz.detach()[:N - 7], xyz0[keep])                     # exactly those 7 left
            assert gm.xyz_gradient_accum.shape[0] == N + 7 and float(gm.xyz_gradient_accum.abs().sum()) == 0.0   # statistics restart
        else:
            assert counts == (0, 0, 0) and torch.equal(gm._xyz.detach(), xyz0)


def test_option_off_is_the_old_call_path(gpu, monkeypatch):
    """Option off: a 20-step run with density control on ends with parameters bit-equal to the same run, same seed, made through
    the pre-existing call path - `rasterize_backward` and `add_densification_stats` behind wrappers that do what they did before the
    option existed (an `abs_grad_out` / `camera_grad_out` / `abs_grad` argument that is not None fails their assertion), the backward
    wrapper calling syn3r_raster_backward_f3d itself.  The loss is the L1 term under a `confidence_map` that is non-zero on one half-tile, so that
    the gradients are the same bits in every launch (tests/test_raster_aa_gpu.py's module docstring)."""
    from syn3r_amd import _lib as L
    from syn3r_amd import raster
    from syn3r_amd.gs import Camera, GaussianModel, GSTrainer, OptimizationParams
    N, H, W = 600, 40, 72
    w2c = np.eye(4, dtype=np.float32)
    calls = {"bwd": 0, "stats": 0}

    def old_backward(st, g_color, g_depth=None, g_alpha=None, **kw):
        assert kw.get("abs_grad_out") is None and kw.get("camera_grad_out") is None      # option off: no buffer is ever handed over
        calls["bwd"] += 1
        radii, geom, binning, image = st.tensors[6:]
        lib, dev = L.load(), radii.device
        n, _, M = st.scene[:3]
        gc = g_color.detach().to(torch.float32).contiguous()
        gd = g_depth.detach().to(torch.float32).contiguous() if g_depth is not None else None
        ga = g_alpha.detach().to(torch.float32).contiguous() if g_alpha is not None else None
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        d_m3, d_sc, d_ro, d_op, d_sh, d_m2 = new(n, 3), new(n, 3), new(n, 4), new(n), new(n, M, 3), new(n, 3)
        d_cf = new(n) if st.has_conf else None
        ws = L.workspace(dev, lib.syn3r_raster_backward_workspace_bytes(n), "raster_bwd")
        L.check(lib.syn3r_raster_backward_f3d(
            *st.scene[:3], st.P, *st.scene[3:], st.bg, L.ptr(radii), L.ptr(geom), geom.numel(), st.plist, L.ptr(image), image.numel(),
            L.ptr(gc), L.ptr(gd), L.ptr(ga), L.ptr(d_m3), L.ptr(d_sc), L.ptr(d_ro), L.ptr(d_op), L.ptr(d_sh), L.ptr(d_m2), L.ptr(d_cf),
            L.ptr(ws), ws.numel(), int(st.raw_params), raster._flags(st.settings), L.ptr(st.filter_3D), L.stream_ptr(dev)),
            "syn3r_raster_backward_f3d")
        return d_m3, d_m2, d_sh, d_op.reshape(st.opacity_shape), d_sc, d_ro, d_cf

    new_stats = GaussianModel.add_densification_stats

    def old_stats(self, viewspace_grad, update_filter, radii=None, abs_grad=None):
        assert abs_grad is None
        calls["stats"] += 1
        return new_stats(self, viewspace_grad, update_filter, radii)

    runs = []
    for old in (False, True):
        with monkeypatch.context() as mp:
            if old:
                mp.setattr(raster, "rasterize_backward", old_backward)
                mp.setattr(GaussianModel, "add_densification_stats", old_stats)
            gm, K = make_scene(N, H, W, 7, gpu)
            cmap = torch.zeros(H, W)
            cmap[16:24, 32:48] = 1.0
            cam = Camera.from_w2c(w2c, K, H, W, image=torch.rand(3, H, W, generator=torch.Generator().manual_seed(5)), data_device=gpu,
                                  cam_confidence=0.7, confidence_map=cmap)
            opt = OptimizationParams(iterations=20, lambda_dssim=0.0, densify_from_iter=4, densification_interval=5,
                                     densify_grad_threshold=1e-7, seed=3)
            tr = GSTrainer(gm, [cam], opt)
            tr.training(0, iterations=20)
            torch.cuda.synchronize()
            runs.append([p.detach().clone() for p in gm.parameters()])
    assert calls["bwd"] == 20 and calls["stats"] == 20            # the second run went through the wrappers, every step
    assert runs[0][0].shape[0] != N                                # density control changed the set
    for a, b in zip(*runs):
        assert a.shape == b.shape and torch.equal(a, b)
