"""The fused photometric loss with a per-pixel weight map (`photometric_loss(weight_map=)`, `syn3r_photo_loss_map*`; an extension
of the published 3DGS loss) and the L1 pair with the same map, against float64 autograd and against the entries without a map.

    L = w * [(1 - lam) * mean(m |I - G|) + lam * mean(m (1 - ssim))],   both means over all C*H*W elements

Tolerances are the ones tests/test_train_ops_gpu.py holds for the loss without a map (weights in [0,1] only shrink the terms):
parts[1] 2e-6; parts[2], parts[3] and the loss 2e-5; the gradient rtol 2e-3, atol 2e-7 + 2e-4 max|grad|."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [((3, 37, 53), 0.2),       # not VEC (W % 4 != 0), partial tiles on both axes, 12 tiles dealt to 8 XCDs
          ((3, 40, 72), 0.2),       # VEC, partial tiles
          ((1, 16, 16), 1.0),       # less than one tile, one channel
          ((3, 20, 70), 0.0)]
MAPS = ["random", "rectangle", "random_1hw"]
W_, UP = 0.7, 1.5


def _published_ssim_map(img1, img2):
    """The published 3DGS `ssim()` (utils/loss_utils.py of the 3DGS code base the FSGS trainer builds on) before its mean:
    11x11 Gaussian window, sigma 1.5, conv2d padding 5, groups = channels."""
    import torch.nn.functional as Fn
    g = torch.tensor([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=img1.dtype)
    g = (g / g.sum())[:, None]
    C = img1.shape[0]
    win = (g @ g.t())[None, None].expand(C, 1, 11, 11).contiguous()
    conv = lambda t: Fn.conv2d(t[None], win, padding=5, groups=C)[0]
    mu1, mu2 = conv(img1), conv(img2)
    s1, s2, s12 = conv(img1 * img1) - mu1 * mu1, conv(img2 * img2) - mu2 * mu2, conv(img1 * img2) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def _images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(shape, generator=g)
    b = (a + 0.2 * torch.randn(shape, generator=g)).clamp(0, 1)      # correlated target: SSIM well away from 0
    return a, b


def _make_map(kind, H, W, seed):
    if kind == "rectangle":           # edges off the tile borders, crossing x = 32 and y = 32 (clipped to the image)
        m = torch.zeros(H, W)
        m[7:35, 5:34] = 1.0
        return m
    m = torch.rand(H, W, generator=torch.Generator().manual_seed(100 + seed))
    return m[None] if kind == "random_1hw" else m


_REF = {}


def _reference(shape, lam, kind):
    """float64 autograd on the CPU, computed once per case: (parts [4], grad of UP * loss)."""
    key = (shape, lam, kind)
    if key not in _REF:
        a, b = _images(shape, 11 + shape[1])
        m = _make_map(kind, shape[1], shape[2], shape[1])
        md = m.double().reshape(shape[1], shape[2])
        ad = a.double().requires_grad_(True)
        l1 = (md * (ad - b.double()).abs()).mean()
        ssim = (md * _published_ssim_map(ad, b.double())).mean()
        mean_m = md.mean()
        loss = W_ * ((1 - lam) * l1 + lam * (mean_m - ssim))
        (loss * UP).backward()
        _REF[key] = (a, b, m, [float(loss.detach()), float(l1.detach()), float(ssim.detach()), float(mean_m)], ad.grad.clone())
    return _REF[key]


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("shape,lam", SHAPES)
def test_photo_map_vs_float64_autograd(shape, lam, kind, gpu, measurements):
    from syn3r_amd.gs.train_ops import photometric_loss
    a, b, m, ref, ref_grad = _reference(shape, lam, kind)
    x = a.to(gpu).requires_grad_(True)
    loss, parts = photometric_loss(x, b.to(gpu), lambda_dssim=lam, weight=W_, return_parts=True, weight_map=m.to(gpu))
    (loss * UP).backward()
    assert parts.shape == (4,)
    p = [float(v) for v in parts.cpu()]
    gmax = float(ref_grad.abs().max())
    err = (x.grad.cpu().double() - ref_grad).abs()
    measurements("photo_map_vs_float64", shape=list(shape), lam=lam, map=kind, loss_err=abs(float(loss.detach()) - ref[0]),
                 l1_err=abs(p[1] - ref[1]), ssim_err=abs(p[2] - ref[2]), mean_m_err=abs(p[3] - ref[3]),
                 grad_err=float(err.max()), grad_max=gmax)
    assert float(loss.detach()) == p[0]
    assert abs(p[1] - ref[1]) < 2e-6
    assert abs(p[2] - ref[2]) < 2e-5 and abs(p[3] - ref[3]) < 2e-5
    assert abs(p[0] - ref[0]) < 2e-5
    torch.testing.assert_close(x.grad.cpu(), ref_grad.float(), rtol=2e-3, atol=2e-7 + 2e-4 * gmax)


@pytest.mark.parametrize("shape,lam", SHAPES + [((3, 270, 480), 0.2)])
def test_map_of_ones_is_the_loss_without_a_map(shape, lam, gpu, measurements):
    """A multiplication by 1.0f is exact: the image gradient has the bits of the call without a map."""
    from syn3r_amd.gs.train_ops import photometric_loss
    a, b = _images(shape, 3 + shape[1])
    a, b = a.to(gpu), b.to(gpu)
    x0 = a.clone().requires_grad_(True)
    l0, p0 = photometric_loss(x0, b, lambda_dssim=lam, weight=W_, return_parts=True)
    (l0 * UP).backward()
    x1 = a.clone().requires_grad_(True)
    l1, p1 = photometric_loss(x1, b, lambda_dssim=lam, weight=W_, return_parts=True, weight_map=torch.ones(shape[1:], device=gpu))
    (l1 * UP).backward()
    assert p0.shape == (3,) and p1.shape == (4,)
    d = (p1[:3].double() - p0.double()).abs().cpu()
    measurements("photo_map_ones", shape=list(shape), lam=lam, parts_err=[float(v) for v in d], mean_m_err=abs(float(p1[3]) - 1.0))
    assert torch.equal(x1.grad, x0.grad)
    assert float(d.max()) <= 1e-7 and abs(float(p1[3]) - 1.0) <= 1e-7


@pytest.mark.parametrize("shape,lam", SHAPES)
def test_map_of_zeros_gives_exact_zeros(shape, lam, gpu):
    from syn3r_amd.gs.train_ops import photometric_loss
    a, b = _images(shape, 5 + shape[1])
    x = a.to(gpu).requires_grad_(True)
    loss, parts = photometric_loss(x, b.to(gpu), lambda_dssim=lam, weight=W_, return_parts=True,
                                   weight_map=torch.zeros(shape[1:], device=gpu))
    (loss * UP).backward()
    assert float(loss.detach()) == 0.0 and bool((parts == 0).all())
    assert bool((x.grad == 0).all())


@pytest.mark.parametrize("shape,lam", SHAPES)
def test_constant_map_is_a_scalar_weight(shape, lam, gpu, measurements):
    """The means run over all elements (not over sum(m)): m = 0.5 with w = 0.7 is no map with w = 0.35."""
    from syn3r_amd.gs.train_ops import photometric_loss
    a, b = _images(shape, 7 + shape[1])
    a, b = a.to(gpu), b.to(gpu)
    x0 = a.clone().requires_grad_(True)
    l0, p0 = photometric_loss(x0, b, lambda_dssim=lam, weight=0.35, return_parts=True)
    (l0 * UP).backward()
    x1 = a.clone().requires_grad_(True)
    l1, p1 = photometric_loss(x1, b, lambda_dssim=lam, weight=0.7, return_parts=True,
                              weight_map=torch.full(shape[1:], 0.5, device=gpu))
    (l1 * UP).backward()
    gmax = float(x0.grad.abs().max())
    measurements("photo_map_constant", shape=list(shape), lam=lam, loss_err=abs(float(l1.detach()) - float(l0.detach())),
                 l1_err=abs(float(p1[1]) - 0.5 * float(p0[1])), ssim_err=abs(float(p1[2]) - 0.5 * float(p0[2])),
                 grad_err=float((x1.grad - x0.grad).abs().max()), grad_max=gmax)
    assert abs(float(l1.detach()) - float(l0.detach())) < 2e-5
    assert abs(float(p1[1]) - 0.5 * float(p0[1])) < 2e-6 and abs(float(p1[2]) - 0.5 * float(p0[2])) < 2e-5
    assert abs(float(p1[3]) - 0.5) < 2e-5
    torch.testing.assert_close(x1.grad, x0.grad, rtol=2e-3, atol=2e-7 + 2e-4 * gmax)


@pytest.mark.parametrize("shape", [(3, 37, 53), (3, 270, 480)])
def test_photo_map_step_equals_forward_then_backward(shape, gpu):
    """`syn3r_photo_loss_map_step` leaves the bits of `syn3r_photo_loss_map` + `syn3r_photo_loss_map_backward` in the four scalars
    and in the image gradient - with and without an upstream gradient."""
    from syn3r_amd.gs.train_ops import photometric_loss, photometric_loss_step
    a, b = _images(shape, 3 + shape[1])
    a, b = a.to(gpu), b.to(gpu)
    m = _make_map("random", shape[1], shape[2], 1).to(gpu)
    for up in (None, 1.5):
        x = a.clone().requires_grad_(True)
        loss, parts = photometric_loss(x, b, lambda_dssim=0.2, weight=W_, return_parts=True, weight_map=m)
        (loss if up is None else loss * up).backward()
        go = None if up is None else torch.tensor(up, device=gpu)
        l2, p2, grad = photometric_loss_step(a, b, 0.2, W_, grad_loss=go, weight_map=m)
        assert p2.shape == (4,)
        assert torch.equal(p2, parts) and torch.equal(l2, loss.detach())
        assert torch.equal(grad, x.grad)
    _, p3, _ = photometric_loss_step(a, b, 0.2, W_)
    assert p3.shape == (3,)


@pytest.mark.parametrize("shape", [(3, 37, 53), (3, 64, 48)])
def test_l1_pair_with_a_map(shape, gpu, measurements):
    """`w * (m |a - b|).mean()` in float64 (plane % 4 != 0: the weights wrap inside a group of four; plane % 4 == 0: one
    16-byte load), the step against autograd, and the maps of ones and zeros."""
    from syn3r_amd.gs.train_ops import l1_loss, l1_loss_step
    g = torch.Generator().manual_seed(sum(shape))
    a = torch.rand(shape, generator=g)
    b = torch.rand(shape, generator=g)
    b.view(-1)[::7] = a.view(-1)[::7]                 # exact ties: sign(0) = 0 as torch.sign
    m = torch.rand(shape[1:], generator=g)
    ad = a.double().requires_grad_(True)
    ref = 0.3 * (m.double() * (ad - b.double()).abs()).mean()
    (ref * 2.5).backward()
    bg = b.to(gpu)
    for mm in (m, m[None]):
        x = a.to(gpu).requires_grad_(True)
        loss = l1_loss(x, bg, weight=0.3, weight_map=mm.to(gpu))
        (loss * 2.5).backward()
        assert loss.shape == () and loss.dtype == torch.float32
        measurements("l1_map", shape=list(shape), loss_rel_err=abs(float(loss.detach()) - float(ref.detach())) / float(ref.detach()),
                     grad_err=float((x.grad.cpu().double() - ad.grad).abs().max()), grad_max=float(ad.grad.abs().max()))
        # the bounds of test_l1_loss_forward_backward, plus one rounding of the product m * sign scale
        assert abs(float(loss.detach()) - float(ref.detach())) <= 2e-6 * abs(float(ref.detach()))
        torch.testing.assert_close(x.grad.cpu(), ad.grad.float(), rtol=1e-6, atol=0)
    l2, g2 = l1_loss_step(a.to(gpu), bg, 0.3, grad_loss=torch.tensor(2.5, device=gpu), weight_map=m.to(gpu))
    assert torch.equal(l2, loss.detach()) and torch.equal(g2, x.grad)
    # ones: the bits of the pair without a map; zeros: exact zeros
    x0 = a.to(gpu).requires_grad_(True)
    l0 = l1_loss(x0, bg, weight=0.3)
    l0.backward()
    x1 = a.to(gpu).requires_grad_(True)
    l1 = l1_loss(x1, bg, weight=0.3, weight_map=torch.ones(shape[1:], device=gpu))
    l1.backward()
    assert torch.equal(x1.grad, x0.grad) and abs(float(l1.detach()) - float(l0.detach())) <= 1e-7
    xz = a.to(gpu).requires_grad_(True)
    lz = l1_loss(xz, bg, weight=0.3, weight_map=torch.zeros(shape[1:], device=gpu))
    lz.backward()
    assert float(lz) == 0.0 and bool((xz.grad == 0).all())


def test_map_rejections(gpu):
    import ctypes
    from syn3r_amd import _lib as L
    from syn3r_amd.gs.train_ops import l1_loss, l1_loss_step, photometric_loss, photometric_loss_step
    a, b = _images((3, 20, 24), 1)
    a, b = a.to(gpu), b.to(gpu)
    good = torch.rand(20, 24, device=gpu)
    bad = {"shape": torch.rand(24, 20, device=gpu), "channels": torch.rand(3, 20, 24, device=gpu), "fp16": good.half(),
           "cpu": good.cpu(), "requires_grad": good.clone().requires_grad_(True)}
    for name, m in bad.items():
        for fn in (lambda: photometric_loss(a, b, weight_map=m), lambda: photometric_loss_step(a, b, weight_map=m),
                   lambda: l1_loss(a, b, weight_map=m), lambda: l1_loss_step(a, b, weight_map=m)):
            with pytest.raises(ValueError):
                fn()
    # the raw C entries: a null map is an error with a message, nothing is launched
    lib = L.load()
    ws = torch.empty(lib.syn3r_photo_loss_map_workspace_bytes(3, 20, 24), dtype=torch.uint8, device=gpu)
    assert ws.numel() >= lib.syn3r_photo_loss_workspace_bytes(3, 20, 24) >= 3 * a.numel() * 4
    out, grad = torch.empty(4, device=gpu), torch.empty_like(a)
    lib.syn3r_last_error.restype = ctypes.c_char_p
    st = L.stream_ptr(gpu)
    calls = [lambda m: lib.syn3r_photo_loss_map(L.ptr(a), L.ptr(b), m, 3, 20, 24, 0.2, 1.0, L.ptr(out), L.ptr(ws), ws.numel(), st),
             lambda m: lib.syn3r_photo_loss_map_backward(L.ptr(a), L.ptr(b), m, 3, 20, 24, 0.2, 1.0, None, L.ptr(ws), L.ptr(grad), st),
             lambda m: lib.syn3r_photo_loss_map_step(L.ptr(a), L.ptr(b), m, 3, 20, 24, 0.2, 1.0, None, L.ptr(out), L.ptr(grad), L.ptr(ws),
                                                     ws.numel(), st),
             lambda m: lib.syn3r_l1_loss_map(L.ptr(a), L.ptr(b), m, a.numel(), 480, 1.0, L.ptr(out), L.ptr(ws), ws.numel(), st),
             lambda m: lib.syn3r_l1_loss_map_backward(L.ptr(a), L.ptr(b), m, a.numel(), 480, 1.0, None, L.ptr(grad), st)]
    for call in calls:
        assert call(None) != 0 and b"null map" in lib.syn3r_last_error()
    assert lib.syn3r_photo_loss_map(None, L.ptr(b), L.ptr(good), 3, 20, 24, 0.2, 1.0, L.ptr(out), L.ptr(ws), ws.numel(), st) != 0
    assert b"null" in lib.syn3r_last_error()
    assert lib.syn3r_photo_loss_map(L.ptr(a), L.ptr(b), L.ptr(good), 3, 0, 24, 0.2, 1.0, L.ptr(out), L.ptr(ws), ws.numel(), st) != 0
    assert lib.syn3r_l1_loss_map(L.ptr(a), L.ptr(b), L.ptr(good), a.numel(), 0, 1.0, L.ptr(out), L.ptr(ws), ws.numel(), st) != 0
    assert lib.syn3r_l1_loss_map(L.ptr(a), L.ptr(b), L.ptr(good), a.numel(), 7, 1.0, L.ptr(out), L.ptr(ws), ws.numel(), st) != 0
    assert lib.syn3r_photo_loss_map_workspace_bytes(3, 0, 24) == 0
    torch.cuda.synchronize()
