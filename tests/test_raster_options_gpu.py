"""The rasteriser's per-render options (`abs_grad_out` / `means2D_abs`, `camera_grad_out` / `camera_grad`) are VALUES on one call path:
whatever the combination, `rasterize_backward`, `GaussianRasterizer` and `GSTrainer.train_step` invoke exactly one backward entry, the
one the option table of `rasterize_backward` names, and the gradients do not depend on which one ran.

Scene: raster_aa_ref.SHAPES[1] (300 Gaussians, 33 x 50, confidence, SH degree 1) - both image sides ragged against the 16 x 16 tile,
the smallest shape of the suite with edge tiles, the confidence output and culled Gaussians.  Where two launches are asked for the
SAME BITS the upstream gradient lives on ONE 16 x 8 half-tile (tests/test_raster_aa_gpu.py's module docstring: the blend backward's
float atomics are then ordered)."""
import itertools
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_aa_ref as A  # noqa: E402
from oracle import raster_oracle as RO  # noqa: E402
from raster_direct import half_tile_masks  # noqa: E402

pytestmark = pytest.mark.gpu

N, H, W, CONF, DEG, SCALE = A.SHAPES[1]
ENTRIES = ("syn3r_raster_backward_f3d", "syn3r_raster_backward_abs", "syn3r_raster_backward_cam")
COMBOS = list(itertools.product((False, True), repeat=2))          # (abs buffer, camera buffer)


def expected_entry(with_abs, with_cam):
    return ENTRIES[2] if with_cam else ENTRIES[1] if with_abs else ENTRIES[0]


@pytest.fixture
def entry_calls(monkeypatch):
    """counting wrappers on the three backward entries: -> {entry name: calls so far}"""
    from syn3r_amd import _lib as L
    lib = L.load()
    calls = {name: 0 for name in ENTRIES}
    for name in ENTRIES:
        def counting(*a, _real=getattr(lib, name), _name=name):
            calls[_name] += 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counting, raising=True)
    return calls


def took(calls):
    """the entries called since the last look, as {name: count}; the counters restart"""
    seen = {k: v for k, v in calls.items() if v}
    for k in calls:
        calls[k] = 0
    return seen


def settings(sc, dev):
    from syn3r_amd.raster import GaussianRasterizationSettings
    f = lambda t: t.float().to(dev).contiguous()
    return GaussianRasterizationSettings(H, W, sc["tfx"], sc["tfy"], f(sc["bg"]), 1.0, f(sc["view"]), f(sc["proj"]), DEG, f(sc["campos"]))


def buffers(with_abs, with_cam, dev):
    """handed over full of NaN: every slot has to be written"""
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    return (nan(N, 2) if with_abs else None), (nan(35) if with_cam else None)


def direct(sc, dev, w, with_abs, with_cam):
    from syn3r_amd.raster import rasterize_backward, rasterize_forward
    f = lambda t: t.to(dev, torch.float32).contiguous()
    ab, cb = buffers(with_abs, with_cam, dev)
    with torch.no_grad():
        st = rasterize_forward(f(sc["m"]), f(sc["sh"]), f(sc["o"]), f(sc["s"]), f(sc["q"]), f(sc["cf"]), settings(sc, dev))[4]
        grads = rasterize_backward(st, *w, abs_grad_out=ab, camera_grad_out=cb)
    return grads, ab, cb


def autograd(sc, dev, w, with_abs, with_cam):
    from syn3r_amd.raster import GaussianRasterizer
    f = lambda t: t.to(dev, torch.float32).clone().requires_grad_(True)
    p = {k: f(sc[k]) for k in A.PARAMS + ("cf",)}
    m2 = torch.zeros(N, 3, device=dev, requires_grad=True)
    ab, cb = buffers(with_abs, with_cam, dev)
    color, _, depth, alpha = GaussianRasterizer(settings(sc, dev))(p["m"], m2, p["o"], shs=p["sh"], scales=p["s"], rotations=p["q"],
                                                                   confidence=p["cf"], means2D_abs=ab, camera_grad=cb)
    ((color * w[0]).sum() + (depth * w[1]).sum() + (alpha * w[2]).sum()).backward()
    return (p["m"].grad, m2.grad, p["sh"].grad, p["o"].grad, p["s"].grad, p["q"].grad, p["cf"].grad), ab, cb


def live_half_tile(sc, dev):
    """the loss weights of raster_aa_ref restricted to the first half-tile through which a gradient reaches the Gaussians"""
    wc, wd, wa = (t.to(dev, torch.float32) for t in A.loss_weights(H, W))
    for m in half_tile_masks(H, W, dev):
        w = ((wc * m).contiguous(), (wd * m).contiguous(), (wa * m).contiguous())
        if float(direct(sc, dev, w, False, False)[0][0].abs().max()) > 0:
            return w
    raise AssertionError("no half-tile of the scene sees a Gaussian")


@pytest.mark.parametrize("route", [direct, autograd], ids=["rasterize_backward", "GaussianRasterizer"])
def test_one_entry_per_call_and_the_same_gradients(route, gpu, entry_calls):
    """All four combinations of the two output buffers: exactly one entry is called, the table's; on one live half-tile the seven
    gradients are bit-equal across the four, and the absolute gradient is bit-equal with and without the camera buffer."""
    sc = A.scene(N, H, W, CONF, SCALE)
    w = live_half_tile(sc, gpu)
    took(entry_calls)
    runs = {}
    for with_abs, with_cam in COMBOS:
        runs[with_abs, with_cam] = route(sc, gpu, w, with_abs, with_cam)
        assert took(entry_calls) == {expected_entry(with_abs, with_cam): 1}, (with_abs, with_cam)
    base = runs[False, False][0]
    assert len(base) == 7 and all(g is not None and bool(torch.isfinite(g).all()) for g in base) and float(base[0].abs().max()) > 0
    for combo, (grads, ab, cb) in runs.items():
        assert len(grads) == 7, combo
        for a, b in zip(grads, base):
            assert torch.equal(a, b), combo
    assert torch.equal(runs[True, False][1], runs[True, True][1]) and float(runs[True, True][1].max()) > 0
    assert torch.equal(runs[False, True][2], runs[True, True][2]) and float(runs[True, True][2].abs().max()) > 0


def make_trainer(dev, **opt_kw):
    """300 Gaussians in front of two 33 x 50 cameras (tests/test_pose_trainer_gpu.py's construction at this module's image size)"""
    from syn3r_amd.gs import Camera, GaussianModel, GSTrainer, OptimizationParams
    from syn3r_amd.gs.pose import se3_exp
    m, s, q, o, sh = RO.synthetic_gaussians(N, seed=5, log_scale_mean=np.log(0.04))
    o = o.clamp(1e-3, 1 - 1e-3)
    gm = GaussianModel(m, torch.log(s), q, torch.log(o / (1 - o)), sh[:, :4].contiguous(), sh_degree=DEG, device=dev)
    fx = W / (2 * math.tan(math.radians(30)))
    K = np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], dtype=np.float32)
    gen = torch.Generator().manual_seed(11)
    cams = [Camera.from_w2c(se3_exp(xi).astype(np.float32), K, H, W, image=torch.rand(3, H, W, generator=gen), data_device=dev)
            for xi in ((0.10, -0.05, 0.20, 0.08, -0.12, 0.05), (-0.15, 0.08, 0.10, -0.06, 0.10, -0.04))]
    return GSTrainer(gm, cams, OptimizationParams(iterations=10, **opt_kw)), cams


@pytest.mark.parametrize("abs_on,pose_on", COMBOS)
def test_trainer_steps_take_the_table_s_entry(abs_on, pose_on, gpu, entry_calls):
    """densify_abs_grad x pose_opt: one explicit and one autograd step on the camera that is not the fixed first one, density
    control on.  Which entry ran; `viewspace_abs_grad` reaches `DensityControl.control` exactly with the option on; no pose table with
    `pose_opt` off, one count per step with it on."""
    tr, cams = make_trainer(gpu, densify_abs_grad=abs_on, pose_opt=pose_on, pose_opt_interval=1000)
    tr.densify = True
    outs, control = [], tr.density.control

    def spy(out):
        outs.append(out)
        return control(out)
    tr.density.control = spy
    for k, explicit in enumerate((True, False)):
        tr.train_step(cams[1], explicit=explicit)
        assert took(entry_calls) == {expected_entry(abs_on, pose_on): 1}, explicit
        assert len(outs) == k + 1 and ("viewspace_abs_grad" in outs[k]) == abs_on, explicit
        if abs_on:
            assert tuple(outs[k]["viewspace_abs_grad"].shape) == (N, 2) and float(outs[k]["viewspace_abs_grad"].max()) > 0
    torch.cuda.synchronize()
    assert (tr.gaussians.xyz_gradient_accum_abs is not None) == abs_on
    if pose_on:
        assert tuple(tr.pose.table.shape) == (2, 35) and tr.pose.counts == [0, 2] and float(tr.pose.table[1].abs().max()) > 0
    else:
        assert tr.pose.table is None and tr.pose.counts == []
