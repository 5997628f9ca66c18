"""The multi-view photometric reprojection term on the GPU (csrc/reproj.hip; train_ops.photo_reprojection_loss[_step], _records)
against its float64 restatement (tests/reproj_ref.py), per element; exact sums, bit identities, buffers; the abstract descent design
on the operator; and the trainer with the term on.

WHICH PIXELS.  The term is piecewise smooth.  A pixel is left out of the per-pixel comparison when the float64 reference shows it
within a margin of a kink, the margin being SAFETY = 2 x the first-order fp32 rounding error of the quantity concerned (the error
model at the top of tests/reproj_ref.py: U = 2^-24 times operation count and magnitude, written out per quantity):
  ambiguous (state or source may differ): q of ANY source within |dq| of the validity border, X_z within |dX_z| of 0.01, the two
            smallest e_s closer than |de_1| + |de_2|; a >= alpha_min and D > 0 compare the shared fp32 inputs themselves - exact, margin 0;
  unsure (gradient may differ): q of the chosen source within |dq| of a lattice line, a channel difference of it within |dI| of 0.
The left-out share is asserted <= 2 % per case (tests/test_reproj_cpu.py shows the reference alone inside it).  Every other pixel must
be on the reference's source and live / dead state.
BOUNDS, per pixel that is not left out (B_x: SAFETY x the model's first-order error of x):
  e        |e - e_ref| <= B_e + 6 U e_ref                  (6 U: the record word drops e's two lowest mantissa bits, <= 3 ulp)
  g_depth  |g - g_ref| <= w / (N a) B_dz + |g_ref| (k / N + 4 U)      k: ambiguous pixels of the case (N_live may differ by k)
  g_alpha  |g - g_ref| <= z x (the g_depth bound) + 2 U |g_ref|
  loss     |L - L_ref| <= w (sum_live B_e / N + 2 k max e / N + (4 trips + 8) U mean e)    ambiguous pixels: count x max e / N_live,
           once for the sum and once for N; 4 trips + 8: the terms of the longest fixed-order fp32 sum (thread, wave tree, waves)
  parts[2] <= k / (H W) + U,  parts[3] <= 2 k / N + U.
The measured share of each bound is printed, recorded through `measurements` as "reproj_*" and quoted in README / DESIGN.md: at most
0.19 % of a case left out; e 17.6 %, g_depth 18.3 %, g_alpha 18.3 %, loss 0.7 %, mean e 0.3 % of their bounds."""
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import reproj_ref as R
from tests.poison import poisoned

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
U = R.U


def _ops():
    from syn3r_amd.gs import train_ops as T
    return T.photo_reprojection_loss, T.photo_reprojection_loss_step, T.photo_reprojection_records


def _on(c, gpu, unaligned=False):
    """the case's tensors on the device; `unaligned`: depth as a view one float into a larger buffer (the scalar path)"""
    d = c["depth"].to(gpu)
    if unaligned:
        buf = torch.zeros(d.numel() + 1, device=gpu)
        buf[1:] = d.reshape(-1)
        d = buf[1:].view(d.shape)
        assert d.data_ptr() % 16 == 4 and d.is_contiguous()
    return d, c["alpha"].to(gpu), c["target"].to(gpu), [s.to(gpu) for s in c["sources"]], c["views"]


def check_against_ref(label, key, got, weight, measurements, kind):
    """got = (parts, g_depth, g_alpha, e, src) from the device; the comparison of the module docstring -> shares of the bounds"""
    H, W, S, _ = key
    c, r, (amb, unsure) = R.reference(key, weight)
    parts, gd, ga, e, src = (t.detach().cpu() for t in got)
    gd, ga, e = gd.reshape(H, W).double(), ga.reshape(H, W).double(), e.double()
    left = amb | unsure
    assert int(left.sum()) <= R.MAX_LEFT_OUT * H * W, (label, int(left.sum()))
    k = int(amb.sum())
    keep = ~amb
    assert torch.equal(src[keep].long(), r.src[keep]), (label, int((src[keep].long() != r.src[keep]).sum()))
    live = r.live & keep
    n = max(r.n_live, 1.0)
    shares = {}
    b_e = R.SAFETY * r.de + 6 * U * r.e
    shares["e"] = float(((e - r.e).abs()[live] / b_e[live]).max()) if live.any() else 0.0
    assert not e[~r.live & keep].any()
    cmp = r.live & ~left
    w = float(np.float32(weight))
    b_gd = w / (n * r.a.clamp(min=1e-30)) * R.SAFETY * r.ddz + r.g_depth.abs() * (k / n + 4 * U)
    b_ga = r.z * b_gd + 2 * U * r.g_alpha.abs()
    tiny = 1e-300
    shares["g_depth"] = float(((gd - r.g_depth).abs()[cmp] / (b_gd[cmp] + tiny)).max()) if cmp.any() else 0.0
    shares["g_alpha"] = float(((ga - r.g_alpha).abs()[cmp] / (b_ga[cmp] + tiny)).max()) if cmp.any() else 0.0
    dead = ~r.live & keep
    assert not gd[dead].any() and not ga[dead].any(), label
    finite = r.cand[torch.isfinite(r.cand)]
    max_e = float(finite.max()) if finite.numel() else 0.0
    mean_e = r.parts[1]
    b_mean = float((R.SAFETY * r.de)[r.live].sum()) / n + 2 * k * max_e / n + (4 * R.trips(H, W) + 8) * U * mean_e
    b_loss = w * b_mean + U * abs(r.loss)
    p = [float(v) for v in parts.double()]
    shares["loss"] = abs(p[0] - r.parts[0]) / (b_loss + tiny)
    shares["mean_e"] = abs(p[1] - r.parts[1]) / (b_mean + U * mean_e + tiny)
    assert abs(p[2] - r.parts[2]) <= k / (H * W) + U and abs(p[3] - r.parts[3]) <= 2 * k / n + U, (label, p, r.parts)
    print(f"{label}: left out {int(left.sum())} of {H * W} ({k} ambiguous), shares of the bounds {shares}")
    measurements("reproj_op", shape=[H, W], sources=S, kind=kind, trips=R.trips(H, W), left_out=int(left.sum()), **shares)
    for name, v in shares.items():
        assert v <= 1.0, (label, name, v)
    return shares


def _run(key, gpu, weight, unaligned=False):
    _, step, records = _ops()
    c, _, _ = R.reference(key, weight)
    d, a, t, srcs, views = _on(c, gpu, unaligned)
    loss, gd, ga, parts = step(d, a, t, srcs, views, weight, 0.5, return_parts=True)
    e, src = records(d, a, t, srcs, views, 0.5)
    assert gd.shape == d.shape and ga.shape == a.shape and float(loss) == float(parts[0])
    return parts, gd, ga, e, src


# ------------------------------------------------------------------------------------------- 1. per element against float64
@pytest.mark.parametrize("key", R.CASES, ids=lambda k: f"{k[0]}x{k[1]}-S{k[2]}")
def test_per_element_against_float64(key, gpu, measurements):
    check_against_ref(f"reproj {key}", key, _run(key, gpu, 0.7), 0.7, measurements, "aligned")


def test_unaligned_depth_takes_the_scalar_path_with_the_same_bits(gpu, measurements):
    key = (64, 256 + 1, 2, 4)                           # ragged against the 4-wide groups: scalar path whatever the alignment
    check_against_ref(f"reproj {key} unaligned", key, _run(key, gpu, 0.7, unaligned=True), 0.7, measurements, "unaligned")
    # W % 4 == 0: the 16-byte path for aligned planes, the scalar one for a depth view 4 bytes off - the same bits
    key = (36, 52, 4, 9)
    a, b = _run(key, gpu, 0.7), _run(key, gpu, 0.7, unaligned=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c, r, _ = R.reference(key, 0.7)
    assert r.n_live > 0 and float(a[0][0]) > 0


def test_second_grid_trip(gpu, measurements):
    """The first shape past the kernel's own grid cap (kRpMaxBlocks x kRpThreads groups of four pixels): a second trip per thread."""
    H, W = R.SECOND_TRIP
    assert R.trips(H, W) == 2 and R.trips(H - 1, W) == 1
    check_against_ref(f"reproj {R.BIG_CASE} second trip", R.BIG_CASE, _run(R.BIG_CASE, gpu, 1.0), 1.0, measurements, "second_trip")


# ----------------------------------------------------------------------------------------------------------- 2. exact sums
def _exact_design(H, W, gpu):
    """Identity pose, fx = fy = 64 (a power of two: q = p exactly in fp32), I_t = 0, a = 1, D = 1, and I_s = 2^-j in all three
    channels at the first and last pixel of the groups on lane, wave, block and trip boundaries: e = 2^-j there exactly, 0 elsewhere."""
    G = (W + 3) // 4
    groups = H * G
    blocks = min(-(-groups // R.THREADS), R.MAX_BLOCKS)
    marks = [0, 1, 63, 64, 255, 256, groups - 1]
    if groups > blocks * R.THREADS:
        marks += [blocks * R.THREADS - 1, blocks * R.THREADS]
    Is = torch.zeros(3, H, W)
    total, j = 0.0, 1
    for q in sorted(set(m for m in marks if 0 <= m < groups)):
        y, x0 = divmod(q, G)
        for x in {4 * x0, min(4 * x0 + 3, W - 1)}:
            Is[:, y, x] = 2.0 ** -j
            total += 2.0 ** -j
            j += 1
    assert j <= 23                                      # every partial sum of these terms is exact in fp32
    k = np.array([64.0, 64.0, (W - 1) / 2, (H - 1) / 2], dtype=np.float32)
    views = (k, np.concatenate([np.eye(3).reshape(9), np.zeros(3), k]).astype(np.float32)[None])
    ones = torch.ones(H, W, device=gpu)
    return ones, ones.clone(), torch.zeros(3, H, W, device=gpu), [Is.to(gpu)], views, Is[0], total


@pytest.mark.parametrize("shape", [(64, 257), R.SECOND_TRIP], ids=["ragged", "second_trip"])
def test_exact_sums(shape, gpu):
    H, W = shape
    _, step, records = _ops()
    d, a, t, srcs, views, plane, total = _exact_design(H, W, gpu)
    weight = 0.75
    loss, gd, ga, parts = step(d, a, t, srcs, views, weight, 0.5, return_parts=True)
    n = H * W
    want = [np.float32(float(np.float32(weight)) * (total / n)), np.float32(total / n), np.float32(1.0), np.float32(1.0)]
    assert [float(v) for v in parts.cpu()] == [float(v) for v in want]
    e, src = records(d, a, t, srcs, views, 0.5)
    assert torch.equal(e.cpu(), plane) and not src.any()            # every pixel live, on source 0, e exact
    assert not gd.any() and not ga.any()                            # t = 0: no parallax, no gradient


# ------------------------------------------------------------------------------------------------- 3. identities and buffers
def test_step_equals_function_and_repeats_bit_for_bit(gpu):
    loss_fn, step, _ = _ops()
    for key in ((37, 53, 2, 2), (36, 52, 4, 9)):
        c, r, _ = R.reference(key, 0.7)
        d, a, t, srcs, views = _on(c, gpu)
        go = torch.tensor(1.7, device=gpu)
        s1 = step(d, a, t, srcs, views, 0.7, 0.5, grad_loss=go, return_parts=True)
        s2 = step(d, a, t, srcs, views, 0.7, 0.5, grad_loss=go, return_parts=True)
        for x, y in zip(s1, s2):
            assert torch.equal(x, y)
        dd, aa = d.clone().requires_grad_(True), a.clone().requires_grad_(True)
        loss, parts = loss_fn(dd, aa, t, srcs, views, 0.7, 0.5, return_parts=True)
        (loss * 1.7).backward()
        assert torch.equal(loss.detach(), s1[0]) and torch.equal(parts, s1[3])
        assert torch.equal(dd.grad, s1[1]) and torch.equal(aa.grad, s1[2])
        assert float(s1[1].abs().max()) > 0 and float(s1[2].abs().max()) > 0
        # [1,H,W] inputs (the rasteriser's shapes) give [1,H,W] gradients with the same bits
        s3 = step(d[None], a[None], t, srcs, views, 0.7, 0.5, grad_loss=go)
        assert s3[1].shape == (1,) + d.shape and torch.equal(s3[1][0], s1[1]) and torch.equal(s3[2][0], s1[2])


def test_gradients_are_added_to_given_buffers_and_written_everywhere_otherwise(gpu, monkeypatch):
    _, step, _ = _ops()
    key = (37, 53, 2, 2)
    c, r, (amb, _) = R.reference(key, 0.7)
    d, a, t, srcs, views = _on(c, gpu)
    outs = {}
    for byte in (0x00, 0xFF, 0x3C):                     # without buffers every element is written: no trace of what the memory held
        with poisoned(monkeypatch, byte):
            outs[byte] = step(d, a, t, srcs, views, 0.7, 0.5, return_parts=True)
            torch.cuda.synchronize(gpu)
    for byte in (0xFF, 0x3C):
        for x, y in zip(outs[0x00], outs[byte]):
            assert torch.equal(x, y), hex(byte)
    _, gd, ga, _ = outs[0x00]
    dead = (~r.live & ~amb).to(gpu)
    assert bool(dead.any()) and not gd[dead].any() and not ga[dead].any()
    assert bool(torch.isfinite(gd).all()) and bool(torch.isfinite(ga).all())
    # given buffers are ADDED to (each flag on its own), and are what comes back
    g = torch.Generator().manual_seed(3)
    bd, ba = torch.randn(d.shape, generator=g).to(gpu), torch.randn(a.shape, generator=g).to(gpu)
    for use_d, use_a in ((True, True), (True, False), (False, True)):
        xd, xa = bd.clone(), ba.clone()
        _, od, oa = step(d, a, t, srcs, views, 0.7, 0.5, grad_out=xd if use_d else None, grad_alpha_out=xa if use_a else None)
        assert (od is xd) == use_d and (oa is xa) == use_a
        assert torch.equal(od, bd + gd if use_d else gd) and torch.equal(oa, ba + ga if use_a else ga)
    for bad in (bd[:, :-1], bd.double(), bd.t()):
        with pytest.raises(ValueError, match=": grad_out"):
            step(d, a, t, srcs, views, 0.7, 0.5, grad_out=bad)
        with pytest.raises(ValueError, match="grad_alpha_out"):
            step(d, a, t, srcs, views, 0.7, 0.5, grad_alpha_out=bad)


def test_all_dead_input_and_rejections(gpu):
    from syn3r_amd import _lib as L
    loss_fn, step, records = _ops()
    c = R.make_case(20, 28, 2, 1)
    d, a, t, srcs, views = _on(c, gpu)
    loss, gd, ga, parts = step(d, torch.zeros_like(a), t, srcs, views, 1.0, 0.5, return_parts=True)
    assert float(loss) == 0.0 and not parts.any() and not gd.any() and not ga.any()
    e, src = records(d, torch.zeros_like(a), t, srcs, views, 0.5)
    assert not e.any() and bool((src == -1).all())
    # the library's own error for shapes and source counts it refuses
    tiny = R.make_case(2, 2, 1, 3)
    one = lambda x: x[..., :1, :].contiguous()
    td, ta, tt, ts, tv = _on(tiny, gpu)
    with pytest.raises(L.Syn3rError, match="H=1"):
        step(one(td), one(ta), one(tt), [one(ts[0])], tv)
    five = R.make_case(6, 8, 4, 1)
    fd, fa, ft, fs, fv = _on(five, gpu)
    with pytest.raises(L.Syn3rError, match="S=5"):
        step(fd, fa, ft, fs + fs[:1], (fv[0], np.concatenate([fv[1], fv[1][:1]])))
    with pytest.raises(L.Syn3rError, match="S=5"):
        loss_fn(fd, fa, ft, fs + fs[:1], (fv[0], np.concatenate([fv[1], fv[1][:1]])))
    with pytest.raises(ValueError, match="views"):
        step(fd, fa, ft, fs, (fv[0], fv[1][:3]))
    with pytest.raises(ValueError, match="float32"):
        step(fd, fa, ft, fs[:3] + [fs[3][:, :-1]], fv)
    with pytest.raises(L.Syn3rError, match="alpha_min"):
        step(fd, fa, ft, fs, fv, 1.0, 0.0)


# ---------------------------------------------------------------------------------------------------- 4. the descent design
def test_descent_on_the_operator_follows_the_float64_loop(gpu, measurements):
    """tests/test_reproj_cpu.py's design and loop with the operator's g_depth in place of the restatement's: the final mean |z - z*|
    within 5 % of the float64 loop's (the yardstick; the margin is for fp32 sign flips at near-zero channel differences).
    Measured: 0.1611 -> 0.017885 in float64, 0.017830 on the operator, ratio 0.9970."""
    _, step, _ = _ops()
    design = R.plane_design()
    H, W = design["H"], design["W"]
    lr = R.descent_rate(design)
    _, e0, e_ref = R.descend(design, R.ref_step(design), lr)
    assert e_ref < 0.5 * e0
    t, srcs = design["target"].to(gpu), [s.to(gpu) for s in design["sources"]]
    ones = torch.ones(H, W, device=gpu)
    op = lambda z32: step(z32.to(gpu), ones, t, srcs, design["views"], float(H * W), 0.5)[1]
    _, _, e_op = R.descend(design, op, lr)
    ratio = e_op / e_ref
    measurements("reproj_descent", start=e0, float64=e_ref, operator=e_op, ratio=ratio)
    print(f"reproj descent: mean |z - z*| {e0:.5f} -> float64 {e_ref:.6f}, operator {e_op:.6f} (ratio {ratio:.4f})")
    assert abs(ratio - 1.0) <= 0.05


# -------------------------------------------------------------------------------------------------------------- 5. trainer
def _scene(gpu, tmp_path, tag, **opt):
    from syn3r_amd import launch
    args = launch.parse(["--scenes", "synthetic:0", "--model_path", str(tmp_path / tag), "--iterations", "10"])
    sc = launch.synthetic_scene("synthetic:0", args, gpu)
    tr = sc["trainer"]
    for k, v in opt.items():
        setattr(tr.opt, k, v)
    cams = tr.scene.getTrainCameras()
    assert len(cams) == 3 and all(c.original_image.shape == (3, 72, 128) for c in cams)
    return tr, cams, sc


def _spy(monkeypatch):
    """-> the list that receives (g_color, g_depth or None, g_alpha or None) of every `raster.rasterize_backward` call from now on"""
    from syn3r_amd import raster
    seen = []
    real = raster.rasterize_backward

    def spy(st, g_color, g_depth=None, g_alpha=None, **kw):
        seen.append(tuple(None if g is None else g.detach().clone() for g in (g_color, g_depth, g_alpha)))
        return real(st, g_color, g_depth, g_alpha, **kw)
    monkeypatch.setattr(raster, "rasterize_backward", spy)
    return seen


def _step(tr, cam, seen, explicit=True):
    """(loss, g_color, g_depth, g_alpha as handed to the rasteriser's backward - bitwise, they come from fixed-order kernels), and the
    parameter gradients (the rasteriser's backward accumulates with float atomics: equal to rounding)"""
    seen.clear()
    loss, _ = tr._explicit_step(cam) if explicit else tr._autograd_step(cam)
    torch.cuda.synchronize()
    (g_color, g_depth, g_alpha), = seen
    return [loss.detach().clone(), g_color, g_depth, g_alpha], [p.grad.detach().clone() for p in tr.gaussians.parameters()]


def _same(a, b):
    """tests/depth_terms.same with the alpha gradient: the loss and what the rasteriser's backward is handed are equal bit for bit
    (fixed-order kernels), the parameter gradients to rounding (the rasteriser's backward accumulates with float atomics)."""
    for x, y in zip(a[0], b[0]):
        assert (x is None) == (y is None) and (x is None or torch.equal(x.reshape(-1), y.reshape(-1)))
    for x, y in zip(a[1], b[1]):
        assert float((x - y).abs().max()) <= 2e-5 * (float(y.abs().max()) + 1e-20)


# Explicit against autograd route.  On ONE route everything is bitwise (`_same`); between the routes the two renders differ in their
# last bits (torch's activations against the rasteriser's own), so bit equality of the loss and of what `rasterize_backward` is handed
# cannot hold, and tests/test_depth_smooth_gpu.py holds the routes to 1e-6 on the loss and 2e-5 of the largest entry on the parameter
# gradients.  Here the same 2e-5 holds for every pixel, with what this term adds derived from the two renders themselves:
#   - the float64 restatement on EACH route's own render names the pixels within an fp32 margin of a kink (`reproj_ref.kinks`, the
#     margins of the per-element test; a lattice line along an axis whose dq/dz is negligible is no kink - the scene's cameras sit on
#     an x baseline, q_y = y everywhere) and the pixels whose state or source differs BETWEEN the two renders (alpha on either side of
#     alpha_min, say): only those may take the other sign, source or state and are left out of the pixel comparison;
#   - N_live scales every pixel's gradient by 1 / N_live, so when the routes' live counts differ by k (the operator's own parts[2] on
#     each render) a pixel may differ by k / N_live of its own value on top: the k / N of the per-element bound, with the ACTUAL k;
#   - a left-out pixel that did differ by more than that ("flipped") changes the parameter gradients, which are linear in the pixel
#     gradients: by at most its change relative to the largest pixel gradient times the largest entry of the term's own share of that
#     parameter gradient (on - off).  Without a flipped pixel and with k = 0 the parameter gradients are held to the plain 2e-5.
def _agree(a, b, off, refs, counts, measurements):
    """a, b: `_step`-like results of the two routes; off: the same with the term off; refs: the float64 restatement's (ambiguous |
    unsure) mask and chosen source on each route's render; counts: the operator's N_live on each render"""
    loss_a, loss_b = float(a[0][0]), float(b[0][0])
    y = b[0][1]
    assert float((a[0][1] - y).abs().max()) <= 2e-5 * float(y.abs().max())                # g_color: no kinks
    flagged = (refs[0][0] | refs[1][0] | (refs[0][1] != refs[1][1])).reshape(-1)
    k, n = abs(counts[0] - counts[1]), min(counts)
    # (the scene's cameras sit on an x baseline: q_y = y, so the first and the last row lie ON the validity border and are flagged whole)
    width = a[0][1].shape[-1]
    assert int(flagged.sum()) <= 2 * width + R.MAX_LEFT_OUT * flagged.numel()
    flip, worst = 0.0, 0.0
    for x, y in zip(a[0][2:], b[0][2:]):
        x, y = x.reshape(-1).double().cpu(), y.reshape(-1).double().cpu()
        top = float(y.abs().max())
        bound = 2e-5 * top + y.abs() * (k / n)
        over = (x - y).abs() > bound
        assert not bool((over & ~flagged).any()), (int((over & ~flagged).sum()), k, n)
        worst = max(worst, float(((x - y).abs() / bound)[~flagged].max()))
        flip += float(((x - y).abs()[over] / top).sum())                                  # (flagged pixels alone can be here)
    shares = []
    for x, y, z in zip(a[1], b[1], off[1]):
        top, own = float(y.abs().max()) + 1e-20, float((y - z).abs().max())
        bound = 2e-5 * top + (k / n + flip) * own
        shares.append(float((x - y).abs().max()) / bound)
        assert shares[-1] <= 1.0, (shares, k, n, flip)
    assert abs(loss_a - loss_b) <= 1e-6                                                    # (tests/test_depth_smooth_gpu.py's bound)
    measurements("reproj_routes", flagged=int(flagged.sum()), k=k, n_live=n, flipped_weight=flip, pixel_share=worst,
                 parameter_shares=shares, loss_difference=abs(loss_a - loss_b))
    print(f"routes: {int(flagged.sum())} pixels flagged, N_live differs by {k} of {n}, flipped weight {flip:.3e}, pixels use {worst:.3f} of "
          f"their bound, parameter gradients {[round(v, 3) for v in shares]}, loss differs by {abs(loss_a - loss_b):.2e}")


def test_both_routes_hand_the_rasteriser_an_alpha_gradient_and_agree(gpu, tmp_path, monkeypatch, measurements):
    _, step, _ = _ops()
    seen = _spy(monkeypatch)
    res, refs, counts = {}, [], []
    for route in ("explicit", "autograd", "off"):
        tr, cams, _ = _scene(gpu, tmp_path, route, reproj_weight=0.0 if route == "off" else 0.5)
        cam = cams[1]
        seen.clear()
        loss, out = tr._autograd_step(cam) if route == "autograd" else tr._explicit_step(cam)
        torch.cuda.synchronize()
        (g_color, g_depth, g_alpha), = seen
        res[route] = [loss.detach().clone(), g_color, g_depth, g_alpha], [p.grad.detach().clone() for p in tr.gaussians.parameters()]
        if route == "off":
            continue
        # what the rasteriser's backward was handed is the operator's result on this route's own render, bit for bit
        images, views, srcs = tr._reproj_sources(cam)
        assert srcs == [cams[0], cams[2]]
        depth, alpha = out["depth"].detach(), out["alpha"].detach()
        _, want_d, want_a, parts = step(depth, alpha, cam.original_image, images, views, 0.5, 0.5, return_parts=True)
        assert g_depth is not None and g_alpha is not None
        assert torch.equal(g_depth.reshape(-1), want_d.reshape(-1)) and torch.equal(g_alpha.reshape(-1), want_a.reshape(-1))
        assert float(g_depth.abs().max()) > 0 and float(g_alpha.abs().max()) > 0
        r = R.term(depth.cpu(), alpha.cpu(), cam.original_image.cpu(), [i.cpu() for i in images], views, 0.5, 0.5)
        amb, unsure = R.kinks(r, skip_flat_lattice=True)
        refs.append((amb | unsure, r.src))
        counts.append(int(round(float(parts[2]) * depth.numel())))
    off = res["off"]
    _agree(res["explicit"], res["autograd"], off, refs, counts, measurements)
    assert off[0][2] is None and off[0][3] is None and torch.equal(off[0][1], res["explicit"][0][1])
    assert float(res["explicit"][0][0]) > float(off[0][0])
    assert float((off[1][0] - res["explicit"][1][0]).abs().max()) > 1e-3 * float(off[1][0].abs().max())      # it moves the positions


def test_ineligible_steps_are_the_steps_of_a_trainer_without_the_term(gpu, tmp_path, monkeypatch):
    seen = _spy(monkeypatch)
    tr, cams, _ = _scene(gpu, tmp_path, "base")
    base = _step(tr, cams[1], seen)
    assert base[0][2] is None and base[0][3] is None

    def pseudo_target(tr, cams):
        cams[1].is_pseudo = True                        # a target outside "train"

    def no_source(tr, cams):
        for k in (0, 2):                                # the other input views are of another size: no candidate
            cams[k].original_image = cams[k].original_image[:, :, :-4].contiguous()
            cams[k].image_width = 124

    def too_early(tr, cams):
        tr.opt.reproj_from_iter = 5

    for name, change in (("pseudo", pseudo_target), ("no_source", no_source), ("early", too_early)):
        tr, cams, _ = _scene(gpu, tmp_path, name, reproj_weight=0.5)
        change(tr, cams)
        _same(base, _step(tr, cams[1], seen))
    tr, cams, _ = _scene(gpu, tmp_path, "late", reproj_weight=0.5, reproj_from_iter=5)
    tr.iteration = 5
    assert _step(tr, cams[1], seen)[0][3] is not None


def test_term_adds_two_launches_and_none_when_off(gpu, monkeypatch):
    """An eligible explicit step gains exactly the step entry's two launches (three on the autograd route, whose forward is the
    value-only entry), every other kernel is launched as often as with the term off, and off launches nothing of csrc/reproj.hip."""
    from tests import trainer_launches as TL
    monkeypatch.setitem(TL.OPTIONS, "reproj", (dict(reproj_weight=0.5), False, False))
    for route in ("explicit", "autograd"):
        off, on = TL.launches(gpu, route, "off"), TL.launches(gpu, route, "reproj")
        assert not any("reproj" in k for k in off)
        extra = {k: on[k] - off.get(k, 0) for k in on if on[k] != off.get(k, 0)}
        want = {"k_reproj_stats": TL.STEPS, "k_reproj_grad": TL.STEPS}
        if route == "autograd":                         # the Function's forward is the value-only entry: its one-block combine as well,
            want["k_reproj_final"] = TL.STEPS           # as for the other depth terms on this route
        assert extra == want, (route, extra)
        assert set(off) <= set(on)


def test_term_shares_the_depth_buffer_with_the_other_depth_terms(gpu, tmp_path, monkeypatch):
    seen = _spy(monkeypatch)
    got = {}
    for name, kw in (("off", {}), ("reproj", dict(reproj_weight=0.5)), ("smooth", dict(depth_smooth_weight=0.05)),
                     ("global", dict(depth_weight=0.05)), ("all", dict(reproj_weight=0.5, depth_smooth_weight=0.05, depth_weight=0.05))):
        tr, cams, _ = _scene(gpu, tmp_path, name, **kw)
        got[name] = _step(tr, cams[1], seen)[0]
    want = got["global"][2].double() + got["smooth"][2].double() + got["reproj"][2].double()
    assert float((got["all"][2].double() - want).abs().max()) <= 1.2e-7 * float(want.abs().max())
    assert torch.equal(got["all"][3], got["reproj"][3])             # the alpha gradient is the term's own
    assert got["smooth"][3] is None and got["global"][3] is None and got["off"][2] is None
    loss = {k: float(v[0]) for k, v in got.items()}
    assert abs((loss["all"] - loss["off"]) - sum(loss[k] - loss["off"] for k in ("global", "smooth", "reproj"))) <= 1e-5
