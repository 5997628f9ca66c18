"""The edge-aware depth-smoothness term (csrc/depth_smooth.hip; train_ops.depth_edge_weights, depth_smoothness_loss[_step]) against
its float64 restatement (tests/depth_smooth_ref.py), element by element, exact cases, buffers, and the trainer with the term on.

The kernels and the reference read the SAME fp32 values, so the sign of every difference is exact and no element is left out of any
comparison.  Tolerances are derived from the kernels' operations, u = 2^-24 (the fp32 unit roundoff):

SUMS.  A thread adds t = 4 * trips terms per sum (trips from the header's grid rule: blocks = min(ceil(H G / 256), 1024), G =
ceil(W / 4)); the wave tree adds 6 levels, the block 2; a term carries 2 roundings (the difference, the product): the project's bound
B = 2 (t + 10) u relative on each of sum wx|dx|, sum wy|dy|, sum d (all terms >= 0, so sum |term| is the sum).  The rows are then
added in fp64.
LOSS = weight (S_x + S_y) / m in fp64, one fp32 rounding: |error| <= (2 B + 2 u) |loss|; S_x, S_y, m each (B + 2 u).
GRADIENT.  grad_i = weight g [ e_i / m - (S_x + S_y) / (m^2 H W) ] in fp64 with ONE fp32 rounding; e_i (the signed edge sum) is exact
up to fp64.  The first term carries m's error (B), the second (S_x + S_y)'s and twice m's (3 B), the rounding u |grad_i|:
    |error_i| <= c u weight |g| (sum over i's edges of w / (N m) + (S_x + S_y) / (m^2 H W)),   c = 6 (t + 10) + 2
(3 B = 6 (t + 10) u, 1 for the rounding, 1 for the second-order terms.)  With sums that are exact (the powers-of-two cases) c = 2.
WEIGHTS.  arg = gamma ((|a| + |b|) + |c|) / 3: the three differences err by u (|a| + |b| + |c|) together (1), then two additions, one
division and one product (4) of quantities <= |arg| / gamma, hence |arg error| <= 5 u |arg|; expf is documented at 1 ulp = 2 u
relative:
    |error| <= (2 + 5 |arg|) u w (1 + 1e-6)

Measured shares of these bounds (recorded through the `measurements` fixture as "depth_smooth_*") are quoted in the README."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import depth_smooth_ref as R
from tests.depth_terms import prior as _prior, same as _same, scene as _scene, spy_rasterize_backward, step_bits as _step_bits
from tests.poison import PATTERNS, poisoned

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
U = 2.0 ** -24
SRC = (ROOT / "syn3r_amd" / "csrc" / "depth_smooth.hip").read_text()
THREADS = int(re.search(r"constexpr int kDsThreads = (\d+);", SRC).group(1))
MAX_BLOCKS = int(re.search(r"constexpr int kDsMaxBlocks = (\d+);", SRC).group(1))
TERMS_PER_TRIP = 4                                # k_dsmooth_stats: four `sx +=`, four `sy +=`, four `sd +=` per trip
assert SRC.count("sx += ds_sel") == TERMS_PER_TRIP and SRC.count("sy += ds_sel") == TERMS_PER_TRIP

# 1x1 .. 3x5: degenerate directions and ragged groups; 37x53: the scalar path; 40x64: the 16-byte path, one wave per row; 9x260: a row
# across wave and block boundaries
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (37, 53), (40, 64), (9, 260)]


def groups(H, W):
    return H * ((W + 3) // 4)


def trips(H, W):
    blocks = min(max((groups(H, W) + THREADS - 1) // THREADS, 1), MAX_BLOCKS)
    return (groups(H, W) + blocks * THREADS - 1) // (blocks * THREADS)


def second_trip_shape(W=260):
    """The fewest rows of a W-wide image at which the grid rule makes a second trip"""
    G = (W + 3) // 4
    H = MAX_BLOCKS * THREADS // G + 1
    assert trips(H, W) == 2 and trips(H - 1, W) == 1
    return H, W


def sum_bound(H, W):
    return 2.0 * (TERMS_PER_TRIP * trips(H, W) + 10) * U


def grad_c(H, W):
    return 6 * (TERMS_PER_TRIP * trips(H, W) + 10) + 2


def _ops():
    from syn3r_amd.gs import train_ops as T
    return T.depth_edge_weights, T.depth_smoothness_loss, T.depth_smoothness_loss_step


_CASES = {}


def case(H, W, kind, gpu):
    """(depth [1,H,W] fp32 in [0.5, 6], weights [2,H,W] fp32, float64 reference for weight 0.75 - exact in fp32, as every weight
    that is held to a bound here) on the CPU, computed once per (shape, kind) and shared; kind "kernel": the weights kernel's output
    for a random image, "random": uniform in [0, 1]"""
    key = (H, W, kind)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * H + W + (7 if kind == "kernel" else 0))
        d = (0.5 + 5.5 * torch.rand(1, H, W, generator=g)).contiguous()
        if kind == "kernel":
            w = _ops()[0](torch.rand(3, H, W, generator=g).to(gpu), 1.0).cpu()
        else:
            w = torch.rand(2, H, W, generator=g)
        _CASES[key] = (d, w, R.ref_smooth(d, w, 0.75))
    return _CASES[key]


def raw_loss_backward(d, w, weight, gpu, grad_loss=None):
    """syn3r_depth_smooth_loss + syn3r_depth_smooth_loss_backward through the C-ABI itself: (parts, grad)"""
    from syn3r_amd import _lib as L
    lib = L.load()
    H, W = d.shape[-2:]
    ws = torch.zeros(max(lib.syn3r_depth_smooth_workspace_bytes(H, W), 256), dtype=torch.uint8, device=gpu)
    parts = torch.zeros(4, device=gpu)
    grad = torch.zeros_like(d)
    L.check(lib.syn3r_depth_smooth_loss(L.ptr(d), L.ptr(w), H, W, weight, L.ptr(parts), L.ptr(ws), ws.numel(), L.stream_ptr(gpu)), "loss")
    L.check(lib.syn3r_depth_smooth_loss_backward(L.ptr(d), L.ptr(w), H, W, weight, L.ptr(grad_loss), L.ptr(ws), ws.numel(), L.ptr(grad), 0,
                                                 L.stream_ptr(gpu)), "backward")
    return parts, grad


def check_against_ref(name, H, W, parts, grad, ref, weight, c=None, B=None, g=1.0):
    """Every bar of the module docstring on one result; -> the largest measured share of each bound"""
    B = sum_bound(H, W) if B is None else B
    c = grad_c(H, W) if c is None else c
    parts, grad = parts.detach().cpu().double(), grad.detach().cpu().double().reshape(H, W)
    assert torch.isfinite(parts).all() and torch.isfinite(grad).all()
    share = {}
    for k, (key, tol) in enumerate((("loss", 2 * B + 2 * U), ("sx", B + 2 * U), ("sy", B + 2 * U), ("m", B + 2 * U))):
        err, bound = abs(float(parts[k]) - ref[key]), tol * abs(ref[key])
        share[key] = err / bound if bound > 0 else 0.0
        print(f"{name}: {key} {float(parts[k])!r} ref {ref[key]!r} error {err:.3e} bound {bound:.3e}")
        assert err <= bound, (key, float(parts[k]), ref[key], err, bound)
    bound = c * U * weight * abs(g) * (ref["edges"] + ref["mean_term"])
    err = (grad - ref["grad"]).abs()
    share["grad"] = float((err / bound.clamp_min(1e-300)).max()) if bound.numel() and float(bound.max()) > 0 else 0.0
    print(f"{name}: gradient max error {float(err.max()):.3e}, largest share of the per-pixel bound (c = {c}) {share['grad']:.3e}")
    bad = err > bound
    assert not bool(bad.any()), (int(bad.sum()), float(err.max()))
    return share


# ---------------------------------------------------------------- 1. operator against float64
@pytest.mark.parametrize("kind", ["kernel", "random"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_op_matches_float64(shape, kind, gpu, measurements):
    _, smooth, step = _ops()
    H, W = shape
    d, w, ref = case(H, W, kind, gpu)
    dg, wg = d.to(gpu), w.to(gpu)
    parts_a, grad_a = raw_loss_backward(dg, wg, 0.75, gpu)
    loss_b, grad_b, parts_b = step(dg, wg, 0.75, return_parts=True)
    x = dg.clone().requires_grad_(True)
    loss_c, parts_c = smooth(x, wg, 0.75, return_parts=True)
    loss_c.backward()
    assert loss_b.shape == () and loss_b.is_cuda and grad_b.shape == d.shape and x.grad.shape == d.shape
    # the three routes leave the same bits
    for p_, g_ in ((parts_b, grad_b), (parts_c, x.grad)):
        assert torch.equal(parts_a.view(torch.int32), p_.view(torch.int32)) and torch.equal(grad_a.view(torch.int32), g_.view(torch.int32))
    assert torch.equal(loss_c.detach(), parts_a[0]) and torch.equal(loss_b, parts_a[0])
    share = check_against_ref(f"depth_smooth {H}x{W} {kind}", H, W, parts_a, grad_a, ref, 0.75)
    measurements("depth_smooth_op", shape=[H, W], kind=kind, trips=trips(H, W), **share)
    if H == 1 and W == 1:
        assert float(parts_a[0]) == 0.0 and float(grad_a) == 0.0
    if W == 1:
        assert float(parts_a[1]) == 0.0
    if H == 1:
        assert float(parts_a[2]) == 0.0


def test_second_trip_once(gpu, measurements):
    _, _, step = _ops()
    H, W = second_trip_shape()
    d, w, ref = case(H, W, "random", gpu)
    _, grad, parts = step(d.to(gpu), w.to(gpu), 0.75, return_parts=True)
    share = check_against_ref(f"depth_smooth {H}x{W} second trip", H, W, parts, grad, ref, 0.75)
    measurements("depth_smooth_op", shape=[H, W], kind="random", trips=trips(H, W), **share)


# ---------------------------------------------------------------- 2. weights kernel against float64 exp
def _weights_against_ref(name, img, gamma, gpu):
    weights = _ops()[0]
    _, H, W = img.shape
    out = weights(img.to(gpu), gamma)
    assert out.shape == (2, H, W) and out.dtype == torch.float32
    out = out.cpu()
    ref = R.ref_weights(img, gamma)
    assert not out[0, :, W - 1].view(torch.int32).any() and not out[1, H - 1, :].view(torch.int32).any()      # exactly +0
    arg = -torch.log(ref.clamp_min(1e-300))
    bound = (2.0 + 5.0 * arg) * U * ref * (1.0 + 1e-6)
    err = (out.double() - ref).abs()
    assert not bool((err > bound).any()), (name, float(err.max()))
    share = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: weights max error {float(err.max()):.3e}, largest share of the bound {share:.3e}")
    return out, share


@pytest.mark.parametrize("shape", SHAPES + [second_trip_shape()], ids=lambda s: f"{s[0]}x{s[1]}")
def test_weights_match_float64_exp(shape, gpu, measurements):
    H, W = shape
    g = torch.Generator().manual_seed(H * 31 + W)
    _, s1 = _weights_against_ref(f"depth_smooth weights {H}x{W} random", torch.rand(3, H, W, generator=g), 1.0, gpu)
    # planted exact steps: multiples of 1/8 per channel, so every difference is exact and the mean has at most one rounding
    img = torch.randint(0, 9, (3, H, W), generator=g).float() / 8.0
    out, s2 = _weights_against_ref(f"depth_smooth weights {H}x{W} steps", img, 2.5, gpu)
    measurements("depth_smooth_weights", shape=[H, W], random=s1, steps=s2)
    flat = _ops()[0](torch.full((3, H, W), 0.25).to(gpu), 2.5).cpu()
    assert bool((flat[0, :, :W - 1] == 1.0).all()) and bool((flat[1, :H - 1, :] == 1.0).all())
    # gamma 0: no edge awareness
    zero = _ops()[0](img.to(gpu), 0.0).cpu()
    assert bool((zero[0, :, :W - 1] == 1.0).all()) and bool((zero[1, :H - 1, :] == 1.0).all())


# ---------------------------------------------------------------- 3. exact cases
@pytest.mark.parametrize("shape", [(37, 53), (40, 64), (9, 260)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_constant_and_empty_depth(shape, gpu):
    _, smooth, step = _ops()
    H, W = shape
    _, w, _ = case(H, W, "random", gpu)
    wg = w.to(gpu)
    for value in (3.25, 0.0, -2.0):              # constant: loss exactly 0, gradient exactly 0; zero / negative: an empty render
        d = torch.full((1, H, W), value, device=gpu)
        loss, grad, parts = step(d, wg, 0.75, return_parts=True)
        assert float(loss) == 0.0 and not grad.any() and torch.isfinite(parts).all()
        assert float(parts[1]) == 0.0 and float(parts[2]) == 0.0 and float(parts[3]) == float(np.float32(value))
        x = d.clone().requires_grad_(True)
        smooth(x, wg, 0.75).backward()
        assert not x.grad.any()
    # a render that is empty on average but not flat: zero loss, zero gradient, finite parts
    d, _, _ = case(H, W, "random", gpu)
    loss, grad, parts = step(-d.to(gpu), wg, 0.75, return_parts=True)
    assert float(loss) == 0.0 and not grad.any() and torch.isfinite(parts).all() and float(parts[3]) < 0.0 and float(parts[1]) > 0.0
    # accumulate on an empty render leaves the buffer's values
    buf = torch.randn(1, H, W, generator=torch.Generator().manual_seed(1)).to(gpu)
    prev = buf.clone()
    step(-d.to(gpu), wg, 0.75, grad_out=buf)
    assert torch.equal(buf, prev)


def test_ties_contribute_exactly_nothing(gpu):
    _, _, step = _ops()
    H, W = 37, 53
    d, w, _ = case(H, W, "random", gpu)
    d, w = d.clone(), w.clone()
    g = torch.Generator().manual_seed(5)
    tx = torch.rand(H, W - 1, generator=g) < 0.1
    ty = torch.rand(H - 1, W, generator=g) < 0.1
    for y, x in tx.nonzero().tolist():
        d[0, y, x + 1] = d[0, y, x]
    for y, x in ty.nonzero().tolist():
        d[0, y + 1, x] = d[0, y, x]
    tx = d[0, :, 1:] == d[0, :, :-1]              # (later plants may have undone earlier ones: take the ties that stand)
    ty = d[0, 1:, :] == d[0, :-1, :]
    assert int(tx.sum()) > 50 and int(ty.sum()) > 50
    base = step(d.to(gpu), w.to(gpu), 0.75, return_parts=True)
    w2 = w.clone()
    w2[0, :, :-1][tx] = 1.0e30                    # whatever a tied edge weighs
    w2[1, :-1, :][ty] = 3.0e38
    other = step(d.to(gpu), w2.to(gpu), 0.75, return_parts=True)
    for a, b in zip(base, other):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ref = R.ref_smooth(d, w, 0.75)
    check_against_ref("depth_smooth ties", H, W, base[2], base[1], ref, 0.75)


@pytest.mark.parametrize("shape", [(9, 260), (40, 64), second_trip_shape()], ids=lambda s: f"{s[0]}x{s[1]}")
def test_powers_of_two_are_summed_exactly(shape, gpu):
    """Depths in {1, 2, 4} and weights in {1/4, 1/2, 1} at EVERY pixel - every lane, wave, block and trip boundary included: every
    term is a multiple of 1/4, every partial sum an integer multiple of 1/4 below 2^24 / 4, so the three sums are exact and parts
    are the fp32 roundings of the float64 quotients; the gradient is held to c = 2."""
    _, _, step = _ops()
    H, W = shape
    g = torch.Generator().manual_seed(H + W)
    d = (2.0 ** torch.randint(0, 3, (1, H, W), generator=g).float()).contiguous()
    w = (2.0 ** -torch.randint(0, 3, (2, H, W), generator=g).float()).contiguous()
    assert 4 * H * W < 2 ** 24
    _, grad, parts = step(d.to(gpu), w.to(gpu), 1.0, return_parts=True)
    d64, w64 = d[0].double(), w.double()
    SX = float((w64[0, :, :-1] * (d64[:, 1:] - d64[:, :-1]).abs()).sum())
    SY = float((w64[1, :-1, :] * (d64[1:, :] - d64[:-1, :]).abs()).sum())
    sx, sy, m = SX / (H * (W - 1)), SY / ((H - 1) * W), float(d64.sum()) / (H * W)
    want = np.array([(sx + sy) / m, sx, sy, m]).astype(np.float32)
    assert parts.cpu().numpy().tolist() == want.tolist(), (parts.cpu().numpy(), want)
    check_against_ref(f"depth_smooth powers of two {H}x{W}", H, W, parts, grad, R.ref_smooth(d, w, 1.0), 1.0, c=2, B=0.0)


def test_edge_awareness(gpu, measurements):
    """The same depth step costs exp(-gamma g) times as much across an image edge of contrast g as across a flat image"""
    weights, _, step = _ops()
    H, W, k, gamma, contrast = 32, 48, 20, 2.0, 0.375
    d = torch.full((1, H, W), 1.0)
    d[0, :, k + 1:] = 3.0
    flat = torch.full((3, H, W), 0.25)
    edged = flat.clone()
    edged[:, :, k + 1:] += contrast
    l_flat, _, p_flat = step(d.to(gpu), weights(flat.to(gpu), gamma), 1.0, return_parts=True)
    l_edge, _, p_edge = step(d.to(gpu), weights(edged.to(gpu), gamma), 1.0, return_parts=True)
    assert float(p_flat[2]) == 0.0 and float(p_edge[2]) == 0.0 and float(p_flat[3]) == float(p_edge[3])
    ratio, want = float(l_edge) / float(l_flat), math.exp(-gamma * contrast)
    tol = want * ((2.0 + 5.0 * gamma * contrast) * U * (1.0 + 1e-6) + 2.0 * (2.0 * sum_bound(H, W) + 2.0 * U))
    measurements("depth_smooth_edge", ratio=ratio, want=want, share=abs(ratio - want) / tol)
    print(f"depth_smooth edge awareness: ratio {ratio!r}, exp(-gamma g) {want!r}, bound {tol:.3e}")
    assert abs(ratio - want) <= tol


# ---------------------------------------------------------------- 4. buffers
@pytest.mark.parametrize("shape", [(37, 53), (40, 64), (9, 260)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_poisoned_buffers_and_accumulate(shape, gpu, monkeypatch):
    _, _, step = _ops()
    H, W = shape
    d, w, ref = case(H, W, "kernel", gpu)
    d, w = d.to(gpu), w.to(gpu)
    outs = []
    for byte in PATTERNS:
        with poisoned(monkeypatch, byte):
            loss, grad, parts = step(d, w, 0.75, return_parts=True)
            torch.cuda.synchronize()
            assert torch.isfinite(grad).all() and torch.isfinite(parts).all()
            outs.append((loss.clone(), grad, parts))
            # accumulate: previous + term, one fp32 rounding of that sum
            prev = torch.randn(1, H, W, generator=torch.Generator().manual_seed(byte)).to(gpu) * float(grad.abs().max())
            buf = prev.clone()
            loss_a, grad_a = step(d, w, 0.75, grad_out=buf)
            torch.cuda.synchronize()
            assert grad_a.data_ptr() == buf.data_ptr() and torch.equal(loss_a, loss)
            want = prev.double() + grad.double()
            assert bool(((buf.double() - want).abs() <= U * want.abs() * (1.0 + 1e-9)).all())
    for o in outs[1:]:
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs[0], o))
    check_against_ref(f"depth_smooth poisoned {H}x{W}", H, W, outs[0][2], outs[0][1], ref, 0.75)


@pytest.mark.parametrize("shape", [(37, 53), (40, 64), (9, 260)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_absent_column_and_row_are_never_read(shape, gpu):
    _, _, step = _ops()
    H, W = shape
    d, w, _ = case(H, W, "random", gpu)
    base = step(d.to(gpu), w.to(gpu), 0.75, return_parts=True)
    for poison in (float("nan"), float("inf"), -3.0e38, 1.0):
        w2 = w.clone()
        w2[0, :, W - 1] = poison
        w2[1, H - 1, :] = poison
        other = step(d.to(gpu), w2.to(gpu), 0.75, return_parts=True)
        for a, b in zip(base, other):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), poison


@pytest.mark.parametrize("shape", [(37, 53), (40, 64), (9, 260)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_misaligned_views_repeatability_and_grad_loss(shape, gpu):
    weights, smooth, step = _ops()
    H, W = shape
    d, w, _ = case(H, W, "random", gpu)
    d, w = d.to(gpu), w.to(gpu)
    l1, g1, p1 = step(d, w, 0.05, return_parts=True)
    l2, g2, p2 = step(d, w, 0.05, return_parts=True)
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and torch.equal(p1, p2)
    # depth 1 float and the weights 3 floats off a 16-byte boundary, then the accumulated buffer 2 floats off: the aligned path's bits
    buf_d, buf_w, buf_g = torch.zeros(H * W + 1, device=gpu), torch.zeros(2 * H * W + 3, device=gpu), torch.zeros(H * W + 2, device=gpu)
    buf_d[1:] = d.reshape(-1)
    buf_w[3:] = w.reshape(-1)
    dm, wm, gm = buf_d[1:].view(1, H, W), buf_w[3:].view(2, H, W), buf_g[2:].view(1, H, W)
    assert dm.data_ptr() % 16 and wm.data_ptr() % 16 and gm.data_ptr() % 16 and d.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0
    for dd, ww in ((dm, wm), (dm, w), (d, wm)):
        lm, gmis, pm = step(dd, ww, 0.05, return_parts=True)
        assert torch.equal(l1, lm) and torch.equal(g1, gmis) and torch.equal(p1, pm)
    step(d, w, 0.05, grad_out=gm)
    assert torch.equal(gm, g1 + 0.0)
    # the weights kernel on a misaligned image and into nothing special: the aligned call's bits
    img = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)).to(gpu)
    buf_i = torch.zeros(3 * H * W + 1, device=gpu)
    buf_i[1:] = img.reshape(-1)
    assert torch.equal(weights(img, 1.0), weights(buf_i[1:].view(3, H, W), 1.0))
    # grad_loss: a power of two scales exactly; any other value is autograd's upstream scalar, bit for bit
    _, g4 = step(d, w, 0.05, grad_loss=torch.tensor(2.0, device=gpu))
    assert torch.equal(g4, 2.0 * g1)
    x = d.clone().requires_grad_(True)
    (smooth(x, w, 0.05) * 0.37).backward()
    _, g37 = step(d, w, 0.05, grad_loss=torch.tensor(0.37, device=gpu))
    assert torch.equal(x.grad, g37)
    assert float((g37.double() - 0.37 * g1.double()).abs().max()) <= 4 * U * float(g1.abs().max())


def test_op_rejects_bad_arguments(gpu):
    from syn3r_amd import _lib
    weights, smooth, step = _ops()
    d, w = torch.rand(1, 16, 16, device=gpu), torch.rand(2, 16, 16, device=gpu)
    for bad in (torch.rand(2, 16, 17, device=gpu), torch.rand(1, 16, 16, device=gpu), torch.rand(512, device=gpu),
                torch.rand(2, 16, 16, device=gpu).half()):
        with pytest.raises(ValueError):
            smooth(d, bad)
        with pytest.raises(ValueError):
            step(d, bad)
    with pytest.raises(ValueError):
        step(d, w, grad_out=torch.zeros(1, 16, 15, device=gpu))
    with pytest.raises(ValueError):
        weights(torch.rand(1, 16, 16, device=gpu))
    with pytest.raises(_lib.Syn3rError):
        weights(torch.rand(3, 16, 16, device=gpu), -1.0)
    with pytest.raises(_lib.Syn3rError):
        step(d, w, float("nan"))
    with pytest.raises(_lib.Syn3rError):                      # the gradient over the depth itself
        step(d, w, 1.0, grad_out=d)


# ---------------------------------------------------------------- 5. the trainer with the term on
N_T, H_T, W_T = 2000, 48, 64


@pytest.mark.parametrize("weights", [(0.0, 0.0, 0.05), (0.05, 0.05, 0.05)], ids=["smooth", "all_three"])
def test_explicit_step_equals_autograd_step(weights, gpu):
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    N, H, W = N_T, H_T, W_T
    w2c = np.eye(4, dtype=np.float32)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(5))
    _, K = _scene(N, H, W, 7, gpu)
    prior = _prior(H, W, K, gpu)
    res = {}
    for route, sw in (("autograd", weights[2]), ("explicit", weights[2]), ("off", 0.0)):
        gm, K = _scene(N, H, W, 7, gpu)
        cam = Camera.from_w2c(w2c, K, H, W, image=target, data_device=gpu, cam_confidence=0.7, depth_image=prior)
        tr = GSTrainer(gm, [cam], OptimizationParams(iterations=1, depth_weight=weights[0], depth_local_weight=weights[1], depth_patch_size=16,
                                                     depth_smooth_weight=sw))
        loss, _ = tr._autograd_step(cam) if route == "autograd" else tr._explicit_step(cam)
        res[route] = [float(loss.detach())] + [p.grad.detach().clone() for p in gm.parameters()]
    assert abs(res["explicit"][0] - res["autograd"][0]) < 1e-6
    for a, b in zip(res["explicit"][1:], res["autograd"][1:]):
        scale = float(b.abs().max()) + 1e-20
        assert float((a - b).abs().max()) <= 2e-5 * scale, (float((a - b).abs().max()), scale)
    # the term is in the loss and in the gradients
    assert res["off"][0] < res["explicit"][0]
    assert float((res["off"][1] - res["explicit"][1]).abs().max()) > 1e-3 * float(res["explicit"][1].abs().max())


def test_weight_zero_leaves_the_step_unchanged(gpu, monkeypatch):
    """depth_smooth_weight = 0: the explicit step's loss and the gradients it hands the rasteriser are bitwise those of a trainer
    without the option, no weights are computed or cached and depth_net is never called - nor is it with the term ON.  All three
    depth terms on: one depth-gradient buffer, the sum of the three separate ones.  depth_smooth_cameras selects its cameras."""
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    from syn3r_amd.gs import trainer as trainer_module
    seen, computed = spy_rasterize_backward(monkeypatch), []
    real_weights = trainer_module.edge_weights_of_image

    def weights_spy(image, gamma):
        computed.append(float(gamma))
        return real_weights(image, gamma)
    monkeypatch.setattr(trainer_module, "edge_weights_of_image", weights_spy)
    N, H, W = N_T, H_T, W_T
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(2))
    _, K = _scene(N, H, W, 4, gpu)
    prior = _prior(H, W, K, gpu)
    w2c = np.eye(4, dtype=np.float32)
    calls = []

    def depth_net(img):
        calls.append(img.shape)
        return prior.clone()

    def run(opt, pseudo=False, **cam_kw):
        gm, _ = _scene(N, H, W, 4, gpu)
        cam = Camera.from_w2c(w2c, K, H, W, image=target, data_device=gpu, **cam_kw)
        cam.is_pseudo = pseudo
        tr = GSTrainer(gm, [cam], opt)
        tr.depth_net = depth_net
        return tr, cam

    tr, cam = run(OptimizationParams())
    tr.depth_net = None
    base = _step_bits(tr, cam, seen)
    assert base[0][2] is None
    # weight 0, whatever the other two options say: the same bits, nothing computed, nothing cached, no network call
    for opt in (OptimizationParams(depth_smooth_weight=0.0), OptimizationParams(depth_smooth_weight=0.0, depth_smooth_gamma=3.0,
                                                                                  depth_smooth_cameras="pseudo")):
        tr, cam = run(opt)
        _same(base, _step_bits(tr, cam, seen))
        assert not computed and cam._depth_edge_cache is None and not calls and cam.depth_image is None
    # the term on: a depth gradient appears, the weights are computed ONCE, and the prior machinery is still untouched
    tr, cam = run(OptimizationParams(depth_smooth_weight=0.05))
    on = _step_bits(tr, cam, seen)
    assert on[0][2] is not None and torch.equal(on[0][1], base[0][1]) and float(on[0][0]) > float(base[0][0])
    again = _step_bits(tr, cam, seen)
    assert computed == [1.0] and not calls and cam.depth_image is None
    assert torch.equal(on[0][2], again[0][2])
    # ... recomputed when gamma or the image changes, not otherwise; a camera's own planes are never recomputed
    cached = cam._depth_edge_cache[3]
    tr.opt.depth_smooth_gamma = 2.0
    assert tr.depth_edge_weights(cam) is not cached and computed == [1.0, 2.0]
    assert tr.depth_edge_weights(cam) is cam._depth_edge_cache[3] and computed == [1.0, 2.0]
    cam.original_image.mul_(0.5)
    tr.depth_edge_weights(cam)
    cam.original_image = cam.original_image.clone()
    tr.depth_edge_weights(cam)
    assert computed == [1.0, 2.0, 2.0, 2.0]
    cam.depth_edge_weights = torch.ones(2, H, W)
    assert tr.depth_edge_weights(cam) is cam.depth_edge_weights and len(computed) == 4
    # which cameras: a training camera under "pseudo" and a pseudo camera under "train" run the plain step
    for kind, pseudo, acts in (("pseudo", False, False), ("train", True, False), ("pseudo", True, True), ("train", False, True),
                               ("all", True, True)):
        tr, cam = run(OptimizationParams(depth_smooth_weight=0.05, depth_smooth_cameras=kind), pseudo=pseudo)
        bits = _step_bits(tr, cam, seen)
        if acts:
            assert torch.equal(bits[0][2], on[0][2]) and torch.equal(bits[0][0], on[0][0])
        else:
            _same(base, bits)
            assert cam._depth_edge_cache is None
    # all three depth terms: ONE buffer, the sum of the three separate ones
    three = {}
    for name, kw in (("global", dict(depth_weight=0.05)), ("local", dict(depth_local_weight=0.05, depth_patch_size=16)),
                     ("smooth", dict(depth_smooth_weight=0.05)),
                     ("all", dict(depth_weight=0.05, depth_local_weight=0.05, depth_patch_size=16, depth_smooth_weight=0.05))):
        tr, cam = run(OptimizationParams(**kw), depth_image=prior)
        three[name] = _step_bits(tr, cam, seen)[0][2].double()
    assert torch.equal(three["smooth"], on[0][2].double())
    want = three["global"] + three["local"] + three["smooth"]
    assert float((three["all"] - want).abs().max()) <= 1.2e-7 * float(want.abs().max())
    assert not calls


# ---------------------------------------------------------------- 6. outcome
# Chosen on the first GPU run from {0.02, 0.05, 0.1, 0.2, 0.5, 1, 2}: the largest weight whose photometric loss after 300 iterations
# stays within 1.5 x the off run's (0.0016 against 0.0012 - 0.0014; 0.5 doubles it, 2 quadruples it).  README.
SMOOTH_WEIGHT = 0.2


def _roughness(tr, cams):
    """(S_x + S_y) / m of the rendered depth, averaged over the cameras (weight 1: the loss value itself)"""
    _, smooth, _ = _ops()
    vals = []
    with torch.no_grad():
        for c in cams:
            vals.append(float(smooth(tr.render_view(c)["depth"], tr.depth_edge_weights(c), 1.0)))
    return float(np.mean(vals))


def _depth_mae(tr, cams):
    """mean |rendered depth - true depth| over the pixels where the truth cloud is seen (`depth_image` is its disparity, 0 elsewhere)"""
    errs = []
    with torch.no_grad():
        for c in cams:
            ok = c.depth_image > 0
            errs.append(float((tr.render_view(c)["depth"][0][ok] - 1.0 / c.depth_image[ok]).abs().mean()))
    return float(np.mean(errs))


def test_term_lowers_the_depth_roughness(gpu, tmp_path, measurements):
    from syn3r_amd import launch
    res = {}
    for sw in (0.0, SMOOTH_WEIGHT):
        args = launch.parse(["--scenes", "synthetic:0", "--model_path", str(tmp_path / f"w{sw}"), "--iterations", "300"])
        sc = launch.synthetic_scene("synthetic:0", args, gpu)
        tr = sc["trainer"]
        cams = tr.scene.getTrainCameras()
        assert all(c.original_image.shape == (3, 72, 128) for c in cams)
        r0 = _roughness(tr, cams)
        tr.opt.depth_smooth_weight = sw
        tr.training(iterations=300, disable_densification=True)
        with torch.no_grad():
            photo = float(np.mean([float(tr._photo_loss(tr.render_view(c)["render"], c, False)[0]) for c in cams]))
        res[sw] = dict(start=r0, end=_roughness(tr, cams), psnr=tr.evaluate(sc["test_cameras"])["psnr"], psnr_train=tr.evaluate()["psnr"],
                       depth_mae=_depth_mae(tr, cams), photo=photo)
    off, on = res[0.0], res[SMOOTH_WEIGHT]
    measurements("depth_smooth_outcome", weight=SMOOTH_WEIGHT, off=off, on=on)
    print(f"depth_smooth outcome, weight {SMOOTH_WEIGHT}: (S_x + S_y) / m at the start {on['start']:.5f}; after 300 iterations off "
          f"{off['end']:.5f}, on {on['end']:.5f}; held-out PSNR off {off['psnr']:.3f} on {on['psnr']:.3f}; training PSNR off "
          f"{off['psnr_train']:.3f} on {on['psnr_train']:.3f}; depth MAE off {off['depth_mae']:.5f} on {on['depth_mae']:.5f}; "
          f"photometric loss off {off['photo']:.5f} on {on['photo']:.5f}")
    assert off["start"] == on["start"]
    assert on["end"] < off["end"]
