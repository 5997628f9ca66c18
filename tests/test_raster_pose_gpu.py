"""The rasteriser's camera gradient on the HIP path (`rasterize_backward(camera_grad_out=)` = syn3r_raster_backward_cam: the POSE
instances of the projection backward, their block sum and k_camera_grad_finish) against the float64 reference of
tests/raster_pose_ref.py, seen from a rotated and shifted camera.

The bar is the project's rasteriser-gradient bar (tests/test_raster_absgrad_gpu.py, BAR = 2e-3), applied per block of the 35 floats
(view, proj, campos) as max |hip - ref| / max |ref of that block|.

Where a test asks for the SAME BITS from two launches, the upstream gradient is non-zero on ONE 16 x 8 half-tile at a time
(tests/test_raster_aa_gpu.py's module docstring: the blend backward's float atomics are then ordered, so the gradient records are the
same bits in every launch); what is under test there - the block sum and the finishing kernel - adds in a fixed order."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_aa_ref as A  # noqa: E402
import raster_pose_ref as P  # noqa: E402
from raster_direct import half_tile_masks  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = 2e-3          # the project's bar for rasteriser gradients (tests/test_raster_absgrad_gpu.py)
IDS = [f"N{s[0]}_{s[1]}x{s[2]}" for s in A.SHAPES]
UNREAD = [3, 7, 11, 15, 18, 22, 26, 30]       # view: the fourth row; proj: clip z
BLOCKS = (("view", slice(0, 16)), ("proj", slice(16, 32)), ("campos", slice(32, 35)))


def settings(sc, dev, deg, aa=False):
    from syn3r_amd.raster import GaussianRasterizationSettings
    f = lambda t: t.detach().float().to(dev).contiguous()
    return GaussianRasterizationSettings(sc["H"], sc["W"], sc["tfx"], sc["tfy"], f(sc["bg"]), 1.0, f(sc["view"]), f(sc["proj"]), deg,
                                         f(sc["campos"]), False, False, aa)


def forward(sc, dev, deg, mode="plain"):
    from syn3r_amd.raster import rasterize_forward
    f = lambda t: t.to(dev, torch.float32).contiguous()
    cf = f(sc["cf"]) if sc["cf"] is not None else None
    filt = f(sc["f"]) if mode.startswith("filter3d") else None
    with torch.no_grad():
        _, radii, _, _, st = rasterize_forward(f(sc["m"]), f(sc["sh"]), f(sc["o"]), f(sc["s"]), f(sc["q"]), cf,
                                               settings(sc, dev, deg, mode.endswith("antialias")), filter_3D=filt)
    return radii, st


def hip_camera_grad(sc, dev, deg, weights, depth_grad=True, mode="plain", with_abs=False):
    """-> (radii, the 7-tuple, cam [35], abs or None); the buffers are handed over full of NaN: every slot has to be written"""
    from syn3r_amd.raster import rasterize_backward
    radii, st = forward(sc, dev, deg, mode)
    wc, wd, wa = (w.to(dev, torch.float32).contiguous() for w in weights)
    buf = torch.full((35,), float("nan"), device=dev)
    ab = torch.full((sc["N"], 2), float("nan"), device=dev) if with_abs else None
    with torch.no_grad():
        grads = rasterize_backward(st, wc, wd if depth_grad else None, wa, abs_grad_out=ab, camera_grad_out=buf)
    return radii, grads, buf, ab


def compare(got, ref_raw, tag, measurements, **extra):
    """all finite, the eight unread slots exact zeros, each block within the bar of its own largest reference entry"""
    assert got.shape == (35,) and got.dtype == torch.float32
    g = got.cpu().double()
    assert bool(torch.isfinite(g).all()), g
    assert float(g[UNREAD].abs().max()) == 0.0
    assert float(ref_raw[UNREAD].abs().max()) == 0.0
    errs = {}
    for name, sl in BLOCKS:
        top = float(ref_raw[sl].abs().max())
        if top == 0.0:                                  # (degree 0: the colour does not depend on the camera centre)
            assert float(g[sl].abs().max()) == 0.0, (tag, name)
            errs[name] = 0.0
            continue
        errs[name] = float((g[sl] - ref_raw[sl]).abs().max()) / top
    print(tag, extra, "max |hip - ref| / max |ref| per block:", {k: f"{v:.3e}" for k, v in errs.items()})
    measurements("raster_pose", tag=tag, **{"err_" + k: v for k, v in errs.items()}, **extra)
    for name, e in errs.items():
        assert e < BAR, (tag, name, e)
    return errs


def check_visibility(radii, valid, N):
    assert int(((radii > 0).cpu() != valid).sum()) <= 0.01 * N      # (an fp32 radius may land on the other side of an integer)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("depth_grad", [True, False], ids=["depth", "nodepth"])
@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("shape", A.SHAPES, ids=IDS)
def test_camera_gradient_vs_reference(shape, mode, depth_grad, gpu, measurements):
    """The raw 35 floats against autograd of the float64 oracle in its three camera tensors: the STAGED instances in the four modes,
    with and without dL_ddepth, on the three scenes (culled, point-like and needle Gaussians; 33 x 50 is no tile multiple; 300 and
    800 end in a partial block).  Measured on an MI355X (profiles/r14/raster_pose.txt): <= 5.2e-6 of a block's largest entry on every
    scene, mode and instance, so the project's 2e-3 stands."""
    ref = P.reference(shape, mode, depth_grad)
    sc = ref["sc"]
    radii, _, got, _ = hip_camera_grad(sc, gpu, ref["deg"], ref["weights"], depth_grad, mode)
    assert int((~ref["valid"]).sum()) > 0
    check_visibility(radii, ref["valid"], sc["N"])
    compare(got, ref["raw"], mode, measurements, shape=list(shape), depth_grad=depth_grad)


# ---------------------------------------------------------------------------------------------------------------- 2
def _behind_camera(sc, n_last):
    """the last `n_last` Gaussians moved behind the camera (camera-space z = -1), in world coordinates"""
    out = P.subset(sc, slice(0, sc["N"]))
    R, t = sc["w2c"][:3, :3], sc["w2c"][:3, 3]
    pc = out["m"][-n_last:] @ R.t() + t
    pc[:, 2] = -1.0
    out["m"][-n_last:] = (pc - t) @ R
    return out


def _small_cases():
    s0, s1, s2 = (P.scene(s) for s in A.SHAPES)
    one = P.with_camera(A.single_gaussian(4.0, 40, 72))
    sh4 = P.subset(s1, slice(0, s1["N"]))
    sh4["sh"] = sh4["sh"][:, :4].clone()
    return {"one_gaussian_deg0": (one, 0), "N63": (P.subset(s0, slice(0, 63)), A.SHAPES[0][4]),
            "N257": (P.subset(s0, slice(0, 257)), A.SHAPES[0][4]), "last300_culled": (_behind_camera(s2, 300), A.SHAPES[2][4]),
            "sh4_deg1_unstaged": (sh4, 1)}


@pytest.mark.parametrize("case", ["one_gaussian_deg0", "N63", "N257", "last300_culled", "sh4_deg1_unstaged"])
def test_smallest_shapes_of_the_reduction(case, gpu, measurements):
    """Each against its own reference: one Gaussian at SH degree 0 (the campos block exact zeros), less than a wavefront (63), one
    live thread in the second block with culled Gaussians in the first (257), two and a half blocks of culled Gaussians at the end -
    one block all culled - (800, the last 300 behind the camera), and four SH coefficients (the instance that does not stage)."""
    sc, deg = _small_cases()[case]
    ref = P.camera_gradient(sc, deg)
    radii, _, got, _ = hip_camera_grad(sc, gpu, deg, ref["weights"])
    check_visibility(radii, ref["valid"], max(sc["N"], 100))
    if case == "one_gaussian_deg0":
        assert int(radii[0]) > 0 and bool(ref["valid"][0]) and float(got[32:].abs().max()) == 0.0 and float(ref["raw"][32:].abs().max()) == 0.0
    if case == "last300_culled":
        assert int((radii[-300:] > 0).sum()) == 0 and int((~ref["valid"][-300:]).sum()) == 300
    if case == "N257":
        assert int(radii[256]) > 0 and int((radii[:256] <= 0).sum()) >= 10
    assert float(ref["raw"][:32].abs().max()) > 0
    compare(got, ref["raw"], case, measurements)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_raw_route_gives_the_activated_routes_gradient(gpu, measurements):
    """raw = 1 (log-scales, unnormalised quaternions, logits in) against the activated route on the same scene: within the bar of each
    block's largest entry (both also hold the reference); whether they are the same bits is recorded."""
    from syn3r_amd import _lib as L
    from syn3r_amd.raster import rasterize_backward, rasterize_forward
    shape = A.SHAPES[0]
    ref = P.reference(shape)
    sc, deg = ref["sc"], ref["deg"]
    N = sc["N"]
    f = lambda t: t.float().to(gpu).contiguous()
    g = torch.Generator().manual_seed(17)
    m3, sh = f(sc["m"]), f(sc["sh"])
    ls = f(torch.log(sc["s"]))
    rr = f(sc["q"] * (0.5 + 1.5 * torch.rand(N, 1, generator=g, dtype=torch.float64)))
    lg = f(torch.log(sc["o"] / (1.0 - sc["o"]))).reshape(N, 1)
    lib, stream = L.load(), L.stream_ptr(gpu)
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=gpu)
    wc, wd, wa = (f(w) for w in ref["weights"])
    with torch.no_grad():
        s_act, r_act, o_act = new(N, 3), new(N, 4), new(N, 1)
        L.check(lib.syn3r_gaussian_activate(N, L.ptr(ls), L.ptr(rr), L.ptr(lg), L.ptr(s_act), L.ptr(r_act), L.ptr(o_act), stream),
                "gaussian_activate")
        st = settings(sc, gpu, deg)
        *_, s0 = rasterize_forward(m3, sh, o_act, s_act, r_act, None, st)
        *_, s1 = rasterize_forward(m3, sh, lg, ls, rr, None, st, raw_params=True)
        c0, c1 = torch.full((35,), float("nan"), device=gpu), torch.full((35,), float("nan"), device=gpu)
        rasterize_backward(s0, wc, wd, wa, camera_grad_out=c0)
        rasterize_backward(s1, wc, wd, wa, camera_grad_out=c1)
    same = bool(torch.equal(c0, c1))
    rel = {}
    for name, sl in BLOCKS:
        rel[name] = float((c0[sl] - c1[sl]).abs().max()) / float(c0[sl].abs().max())
        assert rel[name] < BAR, (name, rel)
    print("raw route against activated route:", rel, "bit-equal:", same)
    measurements("raster_pose_raw_route", bit_equal=same, **{"rel_" + k: v for k, v in rel.items()})
    compare(c1, ref["raw"], "raw_route", measurements, shape=list(shape))


def _live_half_tiles(sc, dev, deg, weights, n=3):
    """upstream gradients restricted to single half-tiles (the first `n` whose camera gradient is non-zero)"""
    from syn3r_amd.raster import rasterize_backward
    wc, wd, wa = (w.to(dev, torch.float32).contiguous() for w in weights)
    out = []
    for m in half_tile_masks(sc["H"], sc["W"], dev):
        _, st = forward(sc, dev, deg)
        buf = torch.zeros(35, device=dev)
        with torch.no_grad():
            rasterize_backward(st, wc * m, wd * m, wa * m, camera_grad_out=buf)
        if float(buf.abs().max()) > 0:
            out.append((wc * m, wd * m, wa * m))
            if len(out) == n:
                break
    assert len(out) == n
    return out


def test_composition_leaves_every_output_alone(gpu, measurements):
    """On single live half-tiles (the module docstring): with dL_dmeans2D_abs also requested, the camera gradient and the absolute
    gradient are bitwise their stand-alone values, and the seven tensors of rasterize_backward are bitwise those of the call without
    `camera_grad_out`."""
    from syn3r_amd.raster import rasterize_backward
    shape = A.SHAPES[2]
    ref = P.reference(shape)
    sc, deg = ref["sc"], ref["deg"]
    N = sc["N"]
    for k, w in enumerate(_live_half_tiles(sc, gpu, deg, ref["weights"])):
        nan = lambda *s: torch.full(s, float("nan"), device=gpu)
        with torch.no_grad():
            plain = rasterize_backward(forward(sc, gpu, deg)[1], *w)
            cam_only, a_only, cam_both, a_both = nan(35), nan(N, 2), nan(35), nan(N, 2)
            g_cam = rasterize_backward(forward(sc, gpu, deg)[1], *w, camera_grad_out=cam_only)
            g_abs = rasterize_backward(forward(sc, gpu, deg)[1], *w, abs_grad_out=a_only)
            g_both = rasterize_backward(forward(sc, gpu, deg)[1], *w, abs_grad_out=a_both, camera_grad_out=cam_both)
        assert float(cam_only.abs().max()) > 0 and float(a_only.max()) > 0
        assert torch.equal(cam_only, cam_both) and torch.equal(a_only, a_both), k
        for other in (g_cam, g_abs, g_both):
            assert len(other) == len(plain) == 7
            for a, b in zip(other, plain):
                assert (a is None and b is None) or torch.equal(a, b), k


# ---------------------------------------------------------------------------------------------------------------- 4
def test_accumulate_and_determinism(gpu):
    """On single live half-tiles: two calls with accumulate = False are the same bits; a call with accumulate = True onto a known
    fp32 row is row + result with torch's fp32 add, bitwise (the unread slots keep the row's value + 0)."""
    from syn3r_amd.raster import rasterize_backward
    shape = A.SHAPES[0]
    ref = P.reference(shape)
    sc, deg = ref["sc"], ref["deg"]
    row0 = torch.randn(35, generator=torch.Generator().manual_seed(9)).to(gpu) * 3.0
    for w in _live_half_tiles(sc, gpu, deg, ref["weights"]):
        a, b = torch.full((35,), float("nan"), device=gpu), torch.full((35,), float("nan"), device=gpu)
        acc = row0.clone()
        with torch.no_grad():
            rasterize_backward(forward(sc, gpu, deg)[1], *w, camera_grad_out=a)
            rasterize_backward(forward(sc, gpu, deg)[1], *w, camera_grad_out=b, camera_grad_accumulate=False)
            rasterize_backward(forward(sc, gpu, deg)[1], *w, camera_grad_out=acc, camera_grad_accumulate=True)
        assert torch.equal(a, b) and float(a.abs().max()) > 0
        assert torch.equal(acc, row0 + a)
        assert not torch.equal(acc, a)


def test_camera_grad_buffer_is_validated(gpu):
    from syn3r_amd.raster import rasterize_backward
    ref = P.reference(A.SHAPES[1])
    sc = ref["sc"]
    _, st = forward(sc, gpu, ref["deg"])
    wc = ref["weights"][0].float().to(gpu)
    for bad in (torch.zeros(34, device=gpu), torch.zeros(35, device=gpu, dtype=torch.float64), torch.zeros(35),
                torch.zeros(70, device=gpu)[::2], torch.zeros(5, 7, device=gpu)):
        with pytest.raises(ValueError, match="camera_grad_out"):
            rasterize_backward(st, wc, camera_grad_out=bad)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_autograd_route_fills_the_buffer(gpu):
    """`GaussianRasterizer(camera_grad=buf)` then `.backward()`: the explicit route's values, bitwise (one live half-tile), added with
    `camera_grad_accumulate`; the parameters' gradients are those of the render without the buffer."""
    from syn3r_amd.raster import GaussianRasterizer, rasterize_backward
    shape = A.SHAPES[1]
    ref = P.reference(shape)
    sc, deg = ref["sc"], ref["deg"]
    wc, wd, wa = _live_half_tiles(sc, gpu, deg, ref["weights"], n=1)[0]
    f = lambda t: t.to(gpu, torch.float32).clone().requires_grad_(True)

    def run(**kw):
        p = {k: f(sc[k]) for k in A.PARAMS}
        cf = sc["cf"].to(gpu, torch.float32) if sc["cf"] is not None else None
        m2 = torch.zeros(sc["N"], 3, device=gpu, requires_grad=True)
        color, _, depth, alpha = GaussianRasterizer(settings(sc, gpu, deg))(p["m"], m2, p["o"], shs=p["sh"], scales=p["s"],
                                                                             rotations=p["q"], confidence=cf, **kw)
        ((color * wc).sum() + (depth * wd).sum() + (alpha * wa).sum()).backward()
        return [p[k].grad for k in A.PARAMS] + [m2.grad]

    explicit = torch.full((35,), float("nan"), device=gpu)
    with torch.no_grad():
        rasterize_backward(forward(sc, gpu, deg)[1], wc, wd, wa, camera_grad_out=explicit)
    buf = torch.full((35,), float("nan"), device=gpu)
    g_with = run(camera_grad=buf)
    assert torch.equal(buf, explicit) and float(buf.abs().max()) > 0
    g_without = run()
    for a, b in zip(g_with, g_without):
        assert torch.equal(a, b)
    run(camera_grad=buf, camera_grad_accumulate=True)
    assert torch.equal(buf, explicit + explicit)
    with pytest.raises(ValueError, match="camera_grad"):
        run(camera_grad=torch.zeros(35, device=gpu, requires_grad=True))
