"""Mip-Splatting's 3D smoothing filter on the HIP path against the float64 reference of tests/raster_f3d_ref.py: the filter kernel
(syn3r_filter3d_compute), the projection kernels with a filter (syn3r_raster_preprocess_f3d / syn3r_raster_backward_f3d, both routes,
with and without anti-aliasing), "NULL means the `_ex` entries", the trainer's two step paths and its bookkeeping, and the property
the filter exists for.  Every test needs the new entries.

Where a test asks for the SAME BITS of gradients from two launches, the upstream gradient is non-zero on ONE 16 x 8 half-tile at a
time, as in tests/test_raster_aa_gpu.py (its module docstring has the reason: the blend backward's float atomics)."""
import inspect
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_aa_ref as A  # noqa: E402
import raster_f3d_ref as F  # noqa: E402
from raster_direct import half_tile_masks, render_direct  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [f"N{s[0]}_{s[1]}x{s[2]}" for s in A.SHAPES]
ROOT = Path(__file__).resolve().parents[1]


def settings(sc, dev, deg, aa):
    from syn3r_amd.raster import GaussianRasterizationSettings
    f = lambda t: t.float().to(dev)
    return GaussianRasterizationSettings(sc["H"], sc["W"], sc["tfx"], sc["tfy"], f(sc["bg"]), 1.0, f(sc["view"]), f(sc["proj"]), deg,
                                         f(sc["campos"]), False, False, aa)


def hip_forward(sc, dev, deg, aa, filt, raw):
    """-> (color, radii, depth, alpha, state) through rasterize_forward, activated tensors or the raw parameters of F.raw_params"""
    from syn3r_amd.raster import rasterize_forward
    f = lambda t: t.to(dev, torch.float32).contiguous()
    p = F.raw_params(sc) if raw else sc
    cf = f(sc["cf"]) if sc["cf"] is not None else None
    with torch.no_grad():
        return rasterize_forward(f(sc["m"]), f(sc["sh"]), f(p["o"]), f(p["s"]), f(p["q"]), cf, settings(sc, dev, deg, aa), raw_params=raw,
                                 filter_3D=f(filt) if filt is not None else None)


# ---------------------------------------------------------------------------------------------------------------- 1
def filter_case(N, C, seed):
    """Cameras (camera 0: identity at the origin; the others tilted by up to 0.2 rad about x and y, eyes in [-1, 1]^2 x [-3, 0],
    their own focal lengths and image sizes) and points in [-5, 5]^2 x [-8, 9]: behind every camera, outside the 15 % margin and
    inside.  All values are fp32-representable (the kernel and the reference read the same numbers) and no point lies within a
    relative 2e-3 of a visibility threshold of any camera (resampled until so; the test asserts 1e-3 on the reference)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    rows = []
    for c in range(C):
        ax, ay = ((rnd(2) - 0.5) * 0.4).tolist() if c else (0.0, 0.0)
        Rx = torch.tensor([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]], dtype=torch.float64)
        Ry = torch.tensor([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]], dtype=torch.float64)
        R = Rx @ Ry
        eye = torch.stack([2 * rnd(1)[0] - 1, 2 * rnd(1)[0] - 1, -3 * rnd(1)[0]]) if c else torch.zeros(3, dtype=torch.float64)
        W, H = ((64.0, 64.0), (72.0, 40.0), (50.0, 33.0))[c % 3]
        fx = 40.0 + 80.0 * float(rnd(1))
        fy = fx * (0.9 + 0.2 * float(rnd(1)))
        rows.append(torch.cat([torch.cat([R, (-R @ eye)[:, None]], 1).reshape(-1), torch.tensor([fx, fy, W, H], dtype=torch.float64)]))
    table = torch.stack(rows).float().double()
    draw = lambda n: torch.stack([10 * rnd(n) - 5, 10 * rnd(n) - 5, 17 * rnd(n) - 8], 1).float().double()
    pts = draw(N)
    if N == 1:
        pts = torch.tensor([[0.1, 0.0, 4.0]], dtype=torch.float64).float().double()
    for _ in range(50):
        bad = F.filter_reference(pts, table)["margin_n"] < 2e-3
        if not bool(bad.any()):
            break
        pts[bad] = draw(int(bad.sum()))
    return pts, table


@pytest.mark.parametrize("C_", [1, 3, 17])
@pytest.mark.parametrize("N", [1, 255, 257, 1000])
def test_filter_kernel_vs_float64(N, C_, gpu, measurements):
    """Bound per element, stated: |got - ref| <= 16 eps32 (sum_i |row_i| |p_i| + |t|) / z * ref, row / t the z row of the camera
    that gives the Gaussian's minimum z / fx (F.filter_reference["bound"]: the rounding of the fp32 dot product that forms z, with
    room for z / fx, sqrt(variance) and their product); an unseen Gaussian carries the bound of the Gaussian with the largest filter.
    The seen / unseen sets are compared through the values: every reference-unseen entry must be the device's maximum bit for bit,
    every reference-seen entry within its own bound (a Gaussian the device had not seen would hold the maximum instead)."""
    from syn3r_amd.gs.train_ops import compute_filter_3D
    pts, table = filter_case(N, C_, seed=1000 * N + C_)
    ref = F.filter_reference(pts, table)
    assert ref["margin_rel"] >= 1e-3                                   # no fp32 visibility decision can flip
    seen, unseen = ref["seen"], ~ref["seen"]
    if N >= 255:
        assert int((~ref["front_any"]).sum()) > 0                      # behind every camera
        assert int((ref["front_any"] & unseen).sum()) > 0              # in front of one, outside its margin
        assert int(seen.sum()) > N // 20
    else:
        assert bool(seen.all())
    got = compute_filter_3D(pts.float().to(gpu), table.float().to(gpu))
    assert got.shape == (N,) and got.dtype == torch.float32
    got = got.cpu().double()
    assert bool(torch.isfinite(got).all()) and float(got.min()) > 0.0
    rel = (got - ref["filter"]).abs() / ref["filter"]
    worst = float((rel[seen] / ref["bound"][seen]).max())
    print(f"N={N} C={C_}: seen {int(seen.sum())}, max relative error {float(rel.max()):.2e}, worst error / bound {worst:.3f}")
    measurements("filter3d_kernel", N=N, C=C_, max_rel=float(rel.max()), worst_over_bound=worst)
    assert bool((rel[seen] <= ref["bound"][seen]).all())
    if bool(unseen.any()):
        top = int(torch.where(seen, ref["filter"], torch.zeros_like(ref["filter"])).argmax())
        assert bool((got[unseen] == got.max()).all()) and float(got[top]) == float(got.max())
        assert bool((rel[unseen] <= ref["bound"][top]).all())


def test_filter_kernel_nothing_seen(gpu):
    """Every point behind every camera: all filters are zero (never NaN or inf); and one seen point among them lifts all to its filter."""
    from syn3r_amd.gs.train_ops import compute_filter_3D
    _, table = filter_case(300, 3, seed=5)
    g = torch.Generator().manual_seed(6)
    pts = torch.stack([10 * torch.rand(300, generator=g) - 5, 10 * torch.rand(300, generator=g) - 5, -20 + 5 * torch.rand(300, generator=g)], 1)
    assert not bool(F.filter_reference(pts, table)["seen"].any())
    got = compute_filter_3D(pts.to(gpu), table.float().to(gpu))
    assert bool(torch.isfinite(got).all()) and bool((got == 0.0).all())
    pts[257] = torch.tensor([0.0, 0.0, 3.0])
    ref = F.filter_reference(pts, table)
    assert ref["seen"].tolist() == [i == 257 for i in range(300)]
    got = compute_filter_3D(pts.to(gpu), table.float().to(gpu)).cpu()
    assert bool((got == got[257]).all()) and abs(float(got[257]) - float(ref["filter"][257])) <= float(ref["bound"][257] * ref["filter"][257])


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialias"])
@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=IDS)
def test_forward_vs_reference(shape, raw, aa, gpu, measurements):
    """Tolerances: the project's (tests/test_raster_aa_gpu.py) - colour and alpha atol 2e-4, depth atol 1e-3 / rtol 1e-4, radii equal."""
    ref = F.reference(shape, aa)
    sc, deg = ref["sc"], ref["deg"]
    assert sc["dropped"] <= 0.01 * sc["N0"]
    color, radii, depth, alpha, _ = hip_forward(sc, gpu, deg, aa, sc["f"], raw)
    c_off, r_off, _, _, _ = hip_forward(sc, gpu, deg, aa, None, raw)
    err = {k: float((a.cpu().double() - b).abs().max()) for k, a, b in (("color", color, ref["color"]), ("depth", depth, ref["depth"]),
                                                                       ("alpha", alpha, ref["alpha"]))}
    moved = float((color - c_off).abs().max())
    print(shape, "raw" if raw else "activated", "aa" if aa else "plain", "max abs error vs float64:", {k: f"{v:.2e}" for k, v in err.items()},
          f"max |colour with - without filter| = {moved:.3f}, radii changed on {int((radii != r_off).sum())}")
    measurements("raster_f3d_forward", shape=list(shape), raw=raw, aa=aa, moved=moved, **err)
    assert torch.isfinite(color).all() and torch.isfinite(depth).all() and torch.isfinite(alpha).all()
    assert torch.equal(radii.cpu().long(), ref["radii"].long())
    np.testing.assert_allclose(color.cpu().numpy(), ref["color"].numpy(), atol=2e-4)
    np.testing.assert_allclose(alpha.cpu().numpy(), ref["alpha"].numpy(), atol=2e-4)
    np.testing.assert_allclose(depth.cpu().numpy(), ref["depth"].numpy(), atol=1e-3, rtol=1e-4)
    assert moved > 0.04 and int((radii != r_off).sum()) > 0          # (the reference moves by >= 0.08 at every shape)


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialias"])
@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=IDS)
def test_backward_vs_reference_autograd(shape, raw, aa, gpu, measurements):
    """Every gradient (means, scales or log-scales, rotations or raw quaternions, opacity or logit, SH, confidence) against float64
    autograd: the largest error below 2e-3 of the tensor's largest entry (the project's bar); finite on the s = 1e-5 / 1e-6 rows."""
    from syn3r_amd.raster import GaussianRasterizer, rasterize_backward
    ref = F.reference(shape, aa)
    sc, deg = ref["sc"], ref["deg"]
    wc, wd, wa = (w.float().to(gpu) for w in ref["weights"])
    if raw:
        color, radii, depth, alpha, st = hip_forward(sc, gpu, deg, aa, sc["f"], True)
        with torch.no_grad():
            d_m3, d_m2, d_sh, d_op, d_sc, d_ro, d_cf = rasterize_backward(st, wc, wd, wa)
        want = ref["grads_raw"]
    else:
        f = lambda t: t.to(gpu, torch.float32).clone().requires_grad_(True)
        p = {k: f(sc[k]) for k in A.PARAMS}
        p["cf"] = f(sc["cf"]) if sc["cf"] is not None else None
        m2 = torch.zeros(sc["N"], 3, device=gpu, requires_grad=True)
        filt = sc["f"].float().to(gpu).requires_grad_(True)              # the filter is data: it must come back without a gradient
        color, radii, depth, alpha = GaussianRasterizer(settings(sc, gpu, deg, aa))(p["m"], m2, p["o"], shs=p["sh"], scales=p["s"],
                                                                                   rotations=p["q"], confidence=p["cf"], filter_3D=filt)
        ((color * wc).sum() + (depth * wd).sum() + (alpha * wa).sum()).backward()
        assert filt.grad is None
        d_m3, d_m2, d_sh, d_op, d_sc, d_ro = p["m"].grad, m2.grad, p["sh"].grad, p["o"].grad, p["s"].grad, p["q"].grad
        d_cf = p["cf"].grad if p["cf"] is not None else None
        want = ref["grads"]
    got = dict(m=d_m3, s=d_sc, q=d_ro, o=d_op.reshape(-1), sh=d_sh)
    if sc["cf"] is not None:
        got["cf"] = d_cf
    assert set(got) == set(want) == set(A.PARAMS) | ({"cf"} if sc["cf"] is not None else set())
    tiny = (sc["s"].min(dim=1).values <= 1.0001e-5).to(gpu)
    assert int(tiny.sum()) >= 14
    err = {}
    for k, b in want.items():
        a = got[k]
        assert torch.isfinite(a).all() and torch.isfinite(a[tiny]).all(), k
        err[k] = (a.cpu().double() - b).abs().max().item() / (b.abs().max().item() + 1e-12)
    print(shape, "raw" if raw else "activated", "aa" if aa else "plain", "max abs gradient error / max abs reference:",
          {k: f"{v:.2e}" for k, v in err.items()})
    measurements("raster_f3d_backward", shape=list(shape), raw=raw, aa=aa, **err)
    for k, v in err.items():
        assert v < 2e-3, (k, v)
    culled = radii == 0
    assert int(culled.sum()) >= 10
    for k, a in got.items():
        assert float(a[culled].abs().max()) == 0.0, k
    assert d_m2.abs().sum() > 0 and (d_m2[:, 2] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("raw,flags", [(0, 0), (1, 1), (0, 1), (1, 0)], ids=["activated", "raw_antialias", "activated_antialias", "raw"])
def test_null_filter_is_the_ex_entries_bit_for_bit(raw, flags, gpu):
    """`filter3d` = NULL through the `_f3d` entries against the `_ex` entries: colour, depth, alpha, radii and the geometry state
    byte for byte, and - one live half-tile at a time - every gradient bit for bit."""
    from syn3r_amd import _lib as L
    shape = A.SHAPES[1]
    N, H, W, conf, deg, scale = shape
    sc = A.scene(N, H, W, conf, scale)
    lib = L.load()
    old = render_direct(lib, sc, gpu, deg, "ex", raw, flags)
    new = render_direct(lib, sc, gpu, deg, "f3d", raw, flags)
    for a, b in zip(old[:5], new[:5]):
        assert torch.equal(a, b)
    assert int((old[3] > 0).sum()) > N // 2 and int(old[4].count_nonzero()) > 1000
    gen = torch.Generator(device="cpu").manual_seed(29)
    gc, gd, ga = (torch.randn(c, H, W, generator=gen).to(gpu) for c in (3, 1, 1))
    names = ("means3D", "scales", "rotations", "opacities", "shs", "means2D", "confidence")
    seen = torch.zeros(N, dtype=torch.bool, device=gpu)
    for m in half_tile_masks(H, W, gpu):
        g = (gc * m, gd * m, ga * m)
        for name, x, y in zip(names, old[5](*g), new[5](*g)):
            assert torch.equal(x, y), (name, float((x - y).abs().max()))
            if name == "opacities":
                seen |= x != 0
    assert int(seen.sum()) > N // 2


def test_python_surface_without_a_filter_is_unchanged(gpu):
    """`filter_3D=None` through rasterize_forward / GaussianRasterizer is the `_ex` render bit for bit, and a wrong-sized filter is
    refused before any launch."""
    from syn3r_amd import _lib as L
    shape = A.SHAPES[1]
    N, H, W, conf, deg, scale = shape
    sc = A.scene(N, H, W, conf, scale)
    old = render_direct(L.load(), sc, gpu, deg, "ex", 0, 1)
    color, radii, depth, alpha, _ = hip_forward(sc, gpu, deg, True, None, False)
    for a, b in zip(old[:4], (color, depth, alpha, radii)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="filter_3D"):
        hip_forward(sc, gpu, deg, True, torch.ones(N - 1), False)
    with pytest.raises(L.Syn3rError):
        from syn3r_amd.raster import rasterize_forward
        f = lambda t: t.float().to(gpu).contiguous()
        rasterize_forward(f(sc["m"]), f(sc["sh"]), f(sc["o"]), f(sc["s"]), f(sc["q"]), None, settings(sc, gpu, deg, False),
                          filter_3D=torch.ones(N))                       # a CPU tensor: no fallback


# ---------------------------------------------------------------------------------------------------------------- 5, 6
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


def _w2c(tx=0.0, ty=0.0, tz=0.0):
    """world-to-camera of a camera at eye (-tx, -ty, -tz) looking down +z"""
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = (tx, ty, tz)
    return m


POSES = (_w2c(), _w2c(0.3, 0.0, 2.0), _w2c(-0.2, 0.1, -1.0))


def _cameras(dev, K, H, W, maps=False):
    from syn3r_amd.gs import Camera
    cams = []
    for i, pose in enumerate(POSES):
        target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(5 + i))
        cmap = None
        if maps:                                                        # one live half-tile per view: bitwise repeatable gradients
            cmap = torch.zeros(H, W)
            cmap[16:24, 16 * (i + 1):16 * (i + 2)] = 1.0
        cams.append(Camera.from_w2c(pose, K, H, W, image=target, data_device=dev, cam_confidence=0.7, confidence_map=cmap))
    return cams


def _reference_filter(tr):
    rows = [F.camera_row(c.world_view_transform.cpu(), math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5), int(c.image_height), int(c.image_width))
            for c in tr.scene.train_cameras[1.0]]
    return F.filter_reference(tr.gaussians._xyz.detach().cpu(), torch.stack(rows).float(), variance=tr.opt.filter_3d_variance)["filter"]


@pytest.mark.parametrize("aa", [False, True], ids=["plain", "antialias"])
def test_trainer_routes_agree(aa, gpu):
    """`OptimizationParams(filter_3d=True)`: the explicit step and the autograd step agree as tests/test_trainer_gpu.py requires of
    the two paths without the filter (loss 1e-6, gradients 2e-5 of the largest entry); both rendered WITH the filter."""
    from syn3r_amd.gs import GSTrainer, OptimizationParams
    from syn3r_amd.gs.train_ops import photometric_loss
    grads, renders = {}, {}
    for explicit in (False, True):
        gm, K, H, W = _trainer_scene(gpu)
        cams = _cameras(gpu, K, H, W)
        tr = GSTrainer(gm, cams, OptimizationParams(iterations=1, filter_3d=True, antialiasing=aa))
        cam = cams[0]
        if explicit:
            loss, out = tr._explicit_step(cam)
            vs = out["viewspace_grad"]
        else:
            out = tr.render_view(cam)
            loss = photometric_loss(out["render"], cam.original_image, 0.2, 0.7)
            loss.backward()
            vs = out["viewspace_points"].grad
        assert gm.filter_3D is not None and gm.filter_3D.shape == (300,) and tr.filter_3d_computes == 1
        np.testing.assert_allclose(gm.filter_3D.cpu().numpy(), _reference_filter(tr).numpy(), rtol=1e-5)
        grads[explicit] = [float(loss)] + [p.grad.detach().clone() for p in gm.parameters()] + [vs.detach().clone()]
        renders[explicit] = out["render"].detach().clone()
    assert abs(grads[True][0] - grads[False][0]) < 1e-6
    for a, b in zip(grads[True][1:], grads[False][1:]):
        assert a.shape == b.shape and torch.isfinite(a).all() and torch.isfinite(b).all()
        scale = float(b.abs().max()) + 1e-20
        assert float((a - b).abs().max()) <= 2e-5 * scale, (float((a - b).abs().max()), scale)
    # ... and the render is not the unfiltered one
    with torch.no_grad():
        tr.opt.filter_3d = False
        plain = tr.render_view(cam)["render"]
    assert float((plain - renders[True]).abs().max()) > 0.04


def test_trainer_bookkeeping(gpu):
    """When the trainer computes the filter again, and when not."""
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    gm, K, H, W = _trainer_scene(gpu)
    cams = _cameras(gpu, K, H, W)
    tr = GSTrainer(gm, cams, OptimizationParams(iterations=10, filter_3d=True, filter_3d_interval=4))
    assert gm.filter_3D is None and tr.filter_3d_computes == 0
    for k in range(4):                                                   # computed at the top of the first step, then kept
        tr.train_step(cams[k % 3])
        assert tr.filter_3d_computes == 1
    f0 = gm.filter_3D
    assert f0.shape == (300,) and f0.dtype == torch.float32 and f0.is_cuda
    tr.train_step(cams[0])                                               # filter_3d_interval steps have passed: positions moved
    assert tr.filter_3d_computes == 2 and gm.filter_3D is not f0          # (computed BEFORE this step's update: compared below)
    # a view that is NOT a training camera: rendered with the filter the training cameras gave, which stays
    f1 = gm.filter_3D
    close = Camera.from_w2c(_w2c(0.0, 0.0, -1.8), K, H, W, data_device=gpu)
    with torch.no_grad():
        out = tr.render_view(close)
        assert tr.evaluate(cams)["n"] == 3
    assert tr.filter_3d_computes == 2 and gm.filter_3D is f1 and torch.isfinite(out["render"]).all()
    # pseudo-views registered: the camera list is another object, the table has 4 rows
    view = torch.rand(3, H, W, generator=torch.Generator().manual_seed(11))
    tr.update_cameras([view], [_w2c(0.1, -0.1, 0.5)], K, 0.05)
    with torch.no_grad():
        tr.render_view(cams[1])
    assert tr.filter_3d_computes == 3 and tr.filter3d.table.shape == (4, 16) and len(tr.scene.train_cameras[1.0]) == 4
    np.testing.assert_allclose(gm.filter_3D.cpu().numpy(), _reference_filter(tr).numpy(), rtol=1e-5)
    with torch.no_grad():
        tr.render_view(cams[2])
    assert tr.filter_3d_computes == 3
    # the orchestrator's restore of the camera list (another list object of another length)
    tr.scene.train_cameras = {1.0: list(cams)}
    with torch.no_grad():
        tr.render_view(cams[1])
    assert tr.filter_3d_computes == 4 and tr.filter3d.table.shape == (3, 16)
    # density control changes N
    gm.ensure_stats()
    gm.xyz_gradient_accum[:40] = 1.0
    gm.denom[:] = 1.0
    n_clone, n_split, n_prune = tr.densify_and_prune(0.5, 0.0, tr.cameras_extent(), None)
    n = gm._xyz.shape[0]
    assert n_clone + n_split > 0 and n != 300 and gm.filter_3D is None
    tr.train_step(cams[0])
    assert tr.filter_3d_computes == 5 and gm.filter_3D.shape == (n,)
    # a checkpoint carries the filter
    state = gm.capture()
    assert torch.equal(state["filter_3D"], gm.filter_3D)


def test_filter_is_computed_without_a_host_round_trip(gpu):
    """No synchronisation is added to the training loop: the operator's code path holds no host read (checked in its source and in
    the kernel file's host code), and it runs under torch's synchronisation guard."""
    from syn3r_amd.gs import train_ops
    from syn3r_amd.gs.trainer import GSTrainer
    src = inspect.getsource(train_ops.compute_filter_3D)
    for word in (".item(", "nonzero", ".cpu(", ".tolist(", "synchronize", ".numpy(", "float(xyz", "int(xyz"):
        assert word not in src, word
    from syn3r_amd.gs.filter3d import Filter3DCache
    src = inspect.getsource(GSTrainer.ensure_filter_3D) + inspect.getsource(Filter3DCache.ensure)    # the delegation and what it calls
    assert "compute_filter_3D(" in src
    for word in (".item(", "nonzero", ".cpu(", ".tolist(", "synchronize", ".numpy(", ".any(", ".all(", ".max("):
        assert word not in src, word
    hip = (ROOT / "syn3r_amd" / "csrc" / "filter3d.hip").read_text()
    host = hip[hip.index('extern "C" int syn3r_filter3d_compute'):]
    for word in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipMemcpy", "hipEventSynchronize"):
        assert word not in host, word
    pts, table = filter_case(1000, 3, seed=9)
    pts, table = pts.float().to(gpu), table.float().to(gpu)
    train_ops.compute_filter_3D(pts, table)                              # (the workspace exists now)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = train_ops.compute_filter_3D(pts, table)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(out).all())


def test_option_off_runs_are_bit_identical(gpu):
    """`filter_3d=False`: a 20-step run equals the run of a trainer whose options never mention the field, parameter for parameter,
    and no filter appears.  L1 loss under per-view confidence maps with one live half-tile each (bitwise repeatable gradients)."""
    from syn3r_amd.gs import GSTrainer, OptimizationParams
    runs = []
    for opt in (OptimizationParams(iterations=20, lambda_dssim=0.0), OptimizationParams(iterations=20, lambda_dssim=0.0, filter_3d=False)):
        gm, K, H, W = _trainer_scene(gpu)
        tr = GSTrainer(gm, _cameras(gpu, K, H, W, maps=True), opt)
        tr.training(0, iterations=20, disable_densification=True)
        assert gm.filter_3D is None and tr.filter_3d_computes == 0 and "filter_3D" not in gm.capture()
        runs.append([p.detach().clone() for p in gm.parameters()])
    start = _trainer_scene(gpu)[0]
    assert float((runs[0][0] - start._xyz).abs().max()) > 0                # the run trained
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_the_property_a_close_up_shows_no_needle(gpu):
    """One Gaussian of scale 1e-3 at z = 2 under a 64 x 64 training camera, rendered from z = 0.25 (F.property_scene: the opacity is
    0.95 / coef, since under an opacity <= 1 the filtered Gaussian is below the blend's 1/255 cut and nothing is drawn).  With the
    filter the alpha image's per-axis second moment about its centre is at least (filter fx / 0.25)^2 = 12.8 px^2 and within 2 % of
    the float64 reference's (12.83); without the filter it is far below (1.58 px^2 at this opacity; 0.35 px^2 - the dilation's 0.3 -
    at opacity 0.95)."""
    from syn3r_amd.gs.train_ops import compute_filter_3D
    from oracle import raster_oracle as RO
    sc, f_ref, fx, coef = F.property_scene()
    H, W = sc["H"], sc["W"]
    view0, _, _, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float64)
    filt = compute_filter_3D(sc["m"].float().to(gpu), F.camera_row(view0, tfx, tfy, H, W)[None].float().to(gpu))
    assert abs(float(filt[0]) - float(f_ref[0])) <= 1e-5 * float(f_ref[0])
    bound = (float(filt[0]) * fx / F.PROP["z_close"]) ** 2
    with torch.no_grad():
        (_, _, _, a_ref, _), _ = F.rasterize(sc, 0, f_ref, False)
    _, radii, _, a_on, _ = hip_forward(sc, gpu, 0, False, filt.cpu().double(), False)
    _, r_off, _, a_off, _ = hip_forward(sc, gpu, 0, False, None, False)
    phys = dict(sc, o=torch.tensor([0.95], dtype=torch.float64))
    _, _, _, a_phys_on, _ = hip_forward(phys, gpu, 0, False, filt.cpu().double(), False)
    _, _, _, a_phys_off, _ = hip_forward(phys, gpu, 0, False, None, False)
    m_on, m_ref, m_off, m_phys = F.second_moment(a_on), F.second_moment(a_ref), F.second_moment(a_off), F.second_moment(a_phys_off)
    print(f"second moment (px^2): with the filter {m_on:.4f} (float64 {m_ref:.4f}, bound {bound:.4f}); without {m_off:.4f}; "
          f"without, opacity 0.95: {m_phys:.4f}; radii {int(radii[0])} / {int(r_off[0])}")
    assert m_on >= bound
    assert abs(m_on - m_ref) <= 0.02 * m_ref
    assert m_off < bound and m_off < 0.2 * bound
    assert 0.25 < m_phys < 0.45
    assert float(a_phys_on.max()) == 0.0 and int(radii[0]) > int(r_off[0])
