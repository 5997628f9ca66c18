"""Anti-aliased splatting on the HIP path (`GaussianRasterizationSettings.antialiasing`, SYN3R_RASTER_ANTIALIAS of
syn3r_raster_preprocess_ex / syn3r_raster_backward_ex) against the float64 reference of tests/raster_aa_ref.py: forward, backward,
the raw-parameter route, "off means unchanged", the energy of a small splat, the trainer and the argument checks.

Where a test asks for the SAME BITS of gradients from two launches, the upstream gradient is non-zero on ONE 16 x 8 half-tile at a
time (`half_tile_masks`).  The blend backward adds the contributions of a Gaussian with float atomics - in LDS across the two
wavefronts of a tile, in memory across tiles - whose order differs from launch to launch (tests/test_raster_bwd_forms_gpu.py
measures 2.5e-7 of a group's largest gradient between two runs of one binary).  With one live half-tile every other wavefront adds
exact zeros, the live one at most two partial sums per slot (a + b = b + a), so the gradient records - and everything the projection
backward makes of them - are the same bits in every launch, and a difference is a difference of arithmetic.  All half-tiles are
walked, so every visible Gaussian is covered."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_aa_ref as R  # noqa: E402
from raster_direct import half_tile_masks, render_direct  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [f"N{s[0]}_{s[1]}x{s[2]}" for s in R.SHAPES]


def settings(sc, dev, deg, aa, debug=False):
    from syn3r_amd.raster import GaussianRasterizationSettings
    f = lambda t: t.float().to(dev)
    return GaussianRasterizationSettings(sc["H"], sc["W"], sc["tfx"], sc["tfy"], f(sc["bg"]), 1.0, f(sc["view"]), f(sc["proj"]), deg,
                                         f(sc["campos"]), False, debug, aa)


def hip_render(sc, dev, deg, aa, requires_grad=False, debug=False):
    from syn3r_amd.raster import GaussianRasterizer
    f = lambda t: t.to(dev, torch.float32).clone().requires_grad_(requires_grad)
    p = {k: f(sc[k]) for k in R.PARAMS}
    p["cf"] = f(sc["cf"]) if sc["cf"] is not None else None
    m2 = torch.zeros(sc["N"], 3, device=dev, requires_grad=requires_grad)
    out = GaussianRasterizer(settings(sc, dev, deg, aa, debug))(p["m"], m2, p["o"], shs=p["sh"], scales=p["s"], rotations=p["q"],
                                                                confidence=p["cf"])
    return out, p, m2


# ---------------------------------------------------------------------------------------------------------------- 1, 2
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_forward_vs_reference(shape, gpu, measurements):
    """Measured on an MI355X (profiles/r10/raster_antialias.txt): colour <= 6.4e-7, alpha <= 1.0e-6, depth <= 4.1e-6."""
    from syn3r_amd.raster import _Rasterize
    ref = R.reference(shape)
    sc, deg = ref["sc"], ref["deg"]
    (color, radii, depth, alpha), _, _ = hip_render(sc, gpu, deg, True, debug=True)
    dbg_on = dict(_Rasterize.debug_state)
    (c_off, r_off, d_off, a_off), _, _ = hip_render(sc, gpu, deg, False, debug=True)
    dbg_off = dict(_Rasterize.debug_state)
    err = {k: float((a.cpu().double() - b).abs().max()) for k, a, b in (("color", color, ref["color"]), ("depth", depth, ref["depth"]),
                                                                       ("alpha", alpha, ref["alpha"]))}
    moved = float((color - c_off).abs().max())
    print(shape, "max abs error vs float64:", {k: f"{v:.2e}" for k, v in err.items()}, f"max |colour on - off| = {moved:.3f}")
    measurements("raster_aa_forward", shape=list(shape), moved=moved, **err)
    # conic, radius, tile rectangle and depth key do not depend on the filter
    assert torch.equal(radii, r_off)
    assert dbg_on["num_rendered"] == dbg_off["num_rendered"] > 0
    assert torch.equal(dbg_on["point_list"], dbg_off["point_list"]) and torch.equal(dbg_on["ranges"], dbg_off["ranges"])
    assert torch.equal(dbg_on["depths"][radii > 0], dbg_off["depths"][radii > 0])      # (a culled Gaussian writes no depth)
    assert torch.isfinite(color).all() and torch.isfinite(depth).all() and torch.isfinite(alpha).all()
    # the bars tests/test_raster_gpu.py holds the same quantities to
    np.testing.assert_allclose(color.cpu().numpy(), ref["color"].numpy(), atol=2e-4)
    np.testing.assert_allclose(alpha.cpu().numpy(), ref["alpha"].numpy(), atol=2e-4)
    np.testing.assert_allclose(depth.cpu().numpy(), ref["depth"].numpy(), atol=1e-3, rtol=1e-4)
    assert moved > 0.05          # the reference moves by >= 0.26 at every shape: the filter is exercised


@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_backward_vs_reference_autograd(shape, gpu, measurements):
    """Measured on an MI355X (profiles/r10/raster_antialias.txt): <= 3.7e-6 of the reference's largest entry for every tensor; the
    point-like and flat Gaussians of the scenes push none near the bar."""
    ref = R.reference(shape)
    sc, deg = ref["sc"], ref["deg"]
    wc, wd, wa = (w.float().to(gpu) for w in ref["weights"])
    (color, _, depth, alpha), p, m2 = hip_render(sc, gpu, deg, True, requires_grad=True)
    ((color * wc).sum() + (depth * wd).sum() + (alpha * wa).sum()).backward()
    err = {}
    for k, b in ref["grads"].items():
        a = p[k].grad.cpu().double()
        assert torch.isfinite(a).all(), k
        err[k] = (a - b).abs().max().item() / (b.abs().max().item() + 1e-12)
    print(shape, "max abs gradient error / max abs reference:", {k: f"{v:.2e}" for k, v in err.items()})
    measurements("raster_aa_backward", shape=list(shape), **err)
    assert set(err) == set(R.PARAMS) | ({"cf"} if sc["cf"] is not None else set())
    for k, v in err.items():
        assert v < 2e-3, (k, v)      # the project's bar for these gradients (tests/test_raster_gpu.py)
    # culled Gaussians (behind the camera, off-axis) write zeros
    for k in R.PARAMS:
        assert float(p[k].grad[:10].abs().max()) == 0.0, k
    assert m2.grad is not None and m2.grad.abs().sum() > 0 and (m2.grad[:, 2] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_raw_route_equals_activate_then_rasterise(gpu):
    """The standard tests/test_trainer_gpu.py holds the raw entries to without the filter, with it: image, depth, alpha and radii
    bit for bit; the parameter gradients of a whole-image loss to the noise of the blend backward's atomics (2e-5 of the largest
    entry), culled rows exactly zero on both routes; and, one live half-tile at a time (module docstring), the same bits."""
    from syn3r_amd import _lib as L
    from syn3r_amd.raster import rasterize_backward, rasterize_forward
    N, H, W, conf, deg, scale = R.SHAPES[0]
    sc = R.scene(N, H, W, True, scale)                      # with a confidence: rho meets it in the blend opacity
    f = lambda t: t.float().to(gpu).contiguous()
    g = torch.Generator().manual_seed(17)
    m3, sh, cf = f(sc["m"]), f(sc["sh"]), f(sc["cf"])
    ls = f(torch.log(sc["s"]))
    rr = f(sc["q"] * (0.5 + 1.5 * torch.rand(N, 1, generator=g, dtype=torch.float64)))      # unnormalised
    lg = f(torch.log(sc["o"] / (1.0 - sc["o"]))).reshape(N, 1)
    st = settings(sc, gpu, deg, True)
    lib, stream = L.load(), L.stream_ptr(gpu)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=gpu)
    with torch.no_grad():
        s_act, r_act, o_act = new(N, 3), new(N, 4), new(N, 1)
        L.check(lib.syn3r_gaussian_activate(N, L.ptr(ls), L.ptr(rr), L.ptr(lg), L.ptr(s_act), L.ptr(r_act), L.ptr(o_act), stream),
                "gaussian_activate")
        *out0, s0 = rasterize_forward(m3, sh, o_act, s_act, r_act, cf, st)
        *out1, s1 = rasterize_forward(m3, sh, lg, ls, rr, cf, st, raw_params=True)
        *out_off, _ = rasterize_forward(m3, sh, lg, ls, rr, cf, settings(sc, gpu, deg, False), raw_params=True)

        def both(gc, gd, ga):
            d_m3, d_m2, d_sh, d_op, d_sc, d_ro, d_cf = rasterize_backward(s0, gc, gd, ga)
            d_ls, d_rr, d_lg = new(N, 3), new(N, 4), new(N, 1)
            L.check(lib.syn3r_gaussian_activate_backward(N, L.ptr(rr), L.ptr(s_act), L.ptr(r_act), L.ptr(o_act), L.ptr(d_sc),
                                                         L.ptr(d_ro), L.ptr(d_op), L.ptr(d_ls), L.ptr(d_rr), L.ptr(d_lg), stream),
                    "gaussian_activate_backward")
            r_m3, r_m2, r_sh, r_lg, r_ls, r_rr, r_cf = rasterize_backward(s1, gc, gd, ga)
            return [d_m3, d_m2, d_sh, d_lg.reshape(-1), d_ls, d_rr, d_cf], [r_m3, r_m2, r_sh, r_lg.reshape(-1), r_ls, r_rr, r_cf]

        for a, b in zip(out0, out1):
            assert torch.equal(a, b)
        assert float((out1[0] - out_off[0]).abs().max()) > 0.05          # the raw route honours the flag
        names = ("xyz", "means2D", "sh", "opacity logit", "log scale", "raw rotation", "confidence")
        gen = torch.Generator(device="cpu").manual_seed(23)
        gc, gd, ga = (torch.randn(c, H, W, generator=gen).to(gpu) for c in (3, 1, 1))
        ref, got = both(gc, gd, ga)
        culled = out0[1] == 0
        assert int(culled.sum()) >= 10 and int((~culled).sum()) > N // 2
        for name, a, b in zip(names, ref, got):
            scale_ = float(a.abs().max()) + 1e-20
            assert float((a - b).abs().max()) <= 2e-5 * scale_, (name, float((a - b).abs().max()), scale_)
            assert float(a[culled].abs().max()) == 0.0 and float(b[culled].abs().max()) == 0.0, name
        seen = torch.zeros(N, dtype=torch.bool, device=gpu)
        for m in half_tile_masks(H, W, gpu):
            ref, got = both(gc * m, gd * m, ga * m)
            for name, a, b in zip(names, ref, got):
                assert torch.equal(a, b), (name, float((a - b).abs().max()))
            seen |= got[3] != 0
        assert int(seen.sum()) > N // 2                                      # the walk reached the visible Gaussians


# ---------------------------------------------------------------------------------------------------------------- 4
def test_filter_off_is_the_old_entries_bit_for_bit(gpu):
    """flags = 0 through the new entries, and antialiasing=False through the Python surface, against the four old entries called
    directly: colour, depth, alpha, radii and - one live half-tile at a time (module docstring) - every gradient, bit for bit."""
    from syn3r_amd import _lib as L
    from syn3r_amd.raster import rasterize_backward, rasterize_forward
    shape = R.SHAPES[1]
    N, H, W, conf, deg, scale = shape
    sc = R.scene(N, H, W, conf, scale)
    lib = L.load()
    old = render_direct(lib, sc, gpu, deg, "plain")
    new = render_direct(lib, sc, gpu, deg, "ex", flags=0)
    f = lambda t: t.float().to(gpu).contiguous()
    with torch.no_grad():
        *py, st = rasterize_forward(f(sc["m"]), f(sc["sh"]), f(sc["o"]), f(sc["s"]), f(sc["q"]), f(sc["cf"]), settings(sc, gpu, deg, False))
    for a, b, c in zip(old[:4], new[:4], (py[0], py[2], py[3], py[1])):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert int((old.radii > 0).sum()) > N // 2
    gen = torch.Generator(device="cpu").manual_seed(29)
    gc, gd, ga = (torch.randn(c, H, W, generator=gen).to(gpu) for c in (3, 1, 1))
    names = ("means3D", "scales", "rotations", "opacities", "shs", "means2D", "confidence")
    seen = torch.zeros(N, dtype=torch.bool, device=gpu)
    for m in half_tile_masks(H, W, gpu):
        g = (gc * m, gd * m, ga * m)
        a = old.backward(*g)
        b = new.backward(*g)
        with torch.no_grad():
            d_m3, d_m2, d_sh, d_op, d_sc, d_ro, d_cf = rasterize_backward(st, *g)
        for name, x, y, z in zip(names, a, b, (d_m3, d_sc, d_ro, d_op, d_sh, d_m2, d_cf)):
            assert torch.equal(x, y), ("_ex, flags = 0", name, float((x - y).abs().max()))
            assert torch.equal(x, z), ("antialiasing=False", name, float((x - z).abs().max()))
        seen |= a[3] != 0
    assert int(seen.sum()) > N // 2


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("z", [2.0, 4.0])
def test_energy_of_a_small_splat_on_the_device(z, gpu):
    sc = R.single_gaussian(z)
    with torch.no_grad():
        (_, _, _, a_ref, _), _, _, _ = R.rasterize(sc, 0, True)
    (_, _, _, alpha), _, _ = hip_render(sc, gpu, 0, True)
    (_, _, _, a_off), _, _ = hip_render(sc, gpu, 0, False)
    fp = R.footprint(sc, z)
    total, total_ref, total_off = float(alpha.double().sum()), float(a_ref.sum()), float(a_off.double().sum())
    print(f"z = {z}: sum(alpha) / footprint = {total / fp:.4f} (reference {total_ref / fp:.4f}; filter off {total_off / fp:.4f})")
    assert abs(total - total_ref) <= 0.02 * total_ref
    assert 0.95 <= total / fp <= 1.01
    assert total_off / fp >= 1.9


# ---------------------------------------------------------------------------------------------------------------- 6
def _trainer_scene(dev, N=300, H=40, W=72, seed=7):
    from oracle import raster_oracle as RO
    from syn3r_amd.gs import GaussianModel
    m, s, q, o, sh = RO.synthetic_gaussians(N, seed=seed, log_scale_mean=np.log(0.03))
    s[10:18] = 1e-5
    logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
    gm = GaussianModel(m, torch.log(s), q, logit, sh, device=dev)
    fx = W / (2 * math.tan(math.radians(30)))
    K = np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], dtype=np.float32)
    return gm, K, H, W


def test_trainer_antialiasing(gpu):
    """`OptimizationParams(antialiasing=True)`: the explicit step and the autograd step agree as tests/test_trainer_gpu.py requires
    of the two paths without the filter (loss 1e-6, gradients 2e-5 of the largest entry), and `render_view` is a direct
    `GaussianRasterizer(antialiasing=True)` render."""
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    from syn3r_amd.gs.train_ops import photometric_loss
    from syn3r_amd.raster import GaussianRasterizationSettings, GaussianRasterizer
    w2c = np.eye(4, dtype=np.float32)
    grads = {}
    for explicit in (False, True):
        gm, K, H, W = _trainer_scene(gpu)
        target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(5))
        cam = Camera.from_w2c(w2c, K, H, W, image=target, data_device=gpu, cam_confidence=0.7)
        tr = GSTrainer(gm, [cam], OptimizationParams(iterations=1, antialiasing=True))
        if explicit:
            loss, out = tr._explicit_step(cam)
            vs = out["viewspace_grad"]
        else:
            out = tr.render_view(cam)
            loss = photometric_loss(out["render"], cam.original_image, 0.2, 0.7)
            loss.backward()
            vs = out["viewspace_points"].grad
        grads[explicit] = [float(loss)] + [p.grad.detach().clone() for p in gm.parameters()] + [vs.detach().clone()]
    assert abs(grads[True][0] - grads[False][0]) < 1e-6
    for a, b in zip(grads[True][1:], grads[False][1:]):
        assert a.shape == b.shape
        scale = float(b.abs().max()) + 1e-20
        assert float((a - b).abs().max()) <= 2e-5 * scale, (float((a - b).abs().max()), scale)
    # render_view = a direct render with the switch on (and not the render without it)
    with torch.no_grad():
        out = tr.render_view(cam)
        renders = {}
        for aa in (True, False):
            st = GaussianRasterizationSettings(
                image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=tr.background,
                scale_modifier=1.0, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
                sh_degree=gm.active_sh_degree, campos=cam.camera_center, prefiltered=False, debug=False, antialiasing=aa)
            renders[aa] = GaussianRasterizer(st)(gm.get_xyz, None, gm.get_opacity, shs=gm.get_features, scales=gm.get_scaling,
                                                 rotations=gm.get_rotation, confidence=gm.confidence)
    color, radii, depth, alpha = renders[True]
    assert torch.equal(out["render"], color) and torch.equal(out["depth"], depth) and torch.equal(out["alpha"], alpha)
    assert torch.equal(out["radii"], radii) and torch.equal(radii, renders[False][1])
    assert float((color - renders[False][0]).abs().max()) > 0.05


def test_trainer_option_off_is_the_step_without_the_field(gpu):
    """`antialiasing=False` against a trainer whose OptimizationParams never mention the field: one explicit step, bit for bit -
    loss, render, gradients and the updated parameters.  The loss is the L1 term under a `confidence_map` that is non-zero on one
    half-tile, so that the gradients are the same bits in every launch (module docstring)."""
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    w2c = np.eye(4, dtype=np.float32)
    runs = []
    for opt in (OptimizationParams(iterations=1, lambda_dssim=0.0), OptimizationParams(iterations=1, lambda_dssim=0.0, antialiasing=False)):
        gm, K, H, W = _trainer_scene(gpu)
        target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(5))
        cmap = torch.zeros(H, W)
        cmap[16:24, 32:48] = 1.0
        cam = Camera.from_w2c(w2c, K, H, W, image=target, data_device=gpu, cam_confidence=0.7, confidence_map=cmap)
        tr = GSTrainer(gm, [cam], opt)
        loss, out = tr._explicit_step(cam)
        g = [p.grad.detach().clone() for p in gm.parameters()]
        tr.optimizer.step()
        runs.append([loss.detach().clone(), out["render"].clone(), out["depth"].clone(), out["radii"].clone()] + g
                    + [p.detach().clone() for p in gm.parameters()])
    assert float(runs[0][4].abs().sum()) > 0                               # the half-tile sees Gaussians
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_unknown_flag_bits_are_rejected_before_any_launch(gpu):
    from syn3r_amd import _lib as L
    shape = R.SHAPES[1]
    N, H, W, conf, deg, scale = shape
    sc = R.scene(N, H, W, conf, scale)
    lib = L.load()
    for bad in (2, 3, 1 << 30, -2):
        with pytest.raises(L.Syn3rError, match="flag"):
            render_direct(lib, sc, gpu, deg, "ex", flags=bad)
    # nothing ran: the output buffers of a refused call keep what they held
    f = lambda t: t.float().to(gpu).contiguous()
    m3, s, q, o, sh, cf = (f(sc[k]) for k in ("m", "s", "q", "o", "sh", "cf"))
    host = lambda t: L.host_f32(t.double().reshape(-1).tolist())
    geom = torch.zeros(lib.syn3r_raster_geom_bytes(N), dtype=torch.uint8, device=gpu)
    radii = torch.full((N,), -7, dtype=torch.int32, device=gpu)
    P = C.c_longlong(-5)
    rc = lib.syn3r_raster_preprocess_ex(N, deg, sh.shape[1], L.ptr(m3), L.ptr(s), L.ptr(q), L.ptr(o), L.ptr(sh), L.ptr(cf), 1.0,
                                        host(sc["view"]), host(sc["proj"]), host(sc["campos"]), float(sc["tfx"]), float(sc["tfy"]), H, W,
                                        L.ptr(radii), L.ptr(geom), geom.numel(), C.byref(P), 0, 2, L.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert rc == -1 and b"flag" in lib.syn3r_last_error()
    assert P.value == -5 and (radii == -7).all() and int(geom.sum()) == 0
    good = render_direct(lib, sc, gpu, deg, "ex", flags=L.RASTER_ANTIALIAS)
    m3_, s_, q_, o_, sh_, cf_, geom_, image_, binning_, ws_ = good.backward.keep
    gc, gd, ga = torch.ones(3, H, W, device=gpu), torch.ones(1, H, W, device=gpu), torch.ones(1, H, W, device=gpu)
    d = [torch.full(shp, -7.0, device=gpu) for shp in ((N, 3), (N, 3), (N, 4), (N,), (N, sh.shape[1], 3), (N, 3), (N,))]
    rc = lib.syn3r_raster_backward_ex(N, deg, sh.shape[1], 1, L.ptr(m3_), L.ptr(s_), L.ptr(q_), L.ptr(o_), L.ptr(sh_), L.ptr(cf_), 1.0,
                                      host(sc["view"]), host(sc["proj"]), host(sc["campos"]), float(sc["tfx"]), float(sc["tfy"]), H, W,
                                      host(sc["bg"]), L.ptr(good.radii), L.ptr(geom_), geom_.numel(), L.ptr(binning_), L.ptr(image_),
                                      image_.numel(), L.ptr(gc), L.ptr(gd), L.ptr(ga), *[L.ptr(t) for t in d], L.ptr(ws_), ws_.numel(),
                                      0, 4, L.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert rc == -1 and b"flag" in lib.syn3r_last_error()
    for t in d:
        assert (t == -7.0).all()
    # and `raw` is 0 or 1
    rc = lib.syn3r_raster_preprocess_ex(N, deg, sh.shape[1], L.ptr(m3), L.ptr(s), L.ptr(q), L.ptr(o), L.ptr(sh), L.ptr(cf), 1.0,
                                        host(sc["view"]), host(sc["proj"]), host(sc["campos"]), float(sc["tfx"]), float(sc["tfy"]), H, W,
                                        L.ptr(radii), L.ptr(geom), geom.numel(), C.byref(P), 2, 0, L.stream_ptr(gpu))
    assert rc == -1 and b"raw" in lib.syn3r_last_error() and (radii == -7).all()
