"""LPIPS (VGG16) loss term on the HIP path against the torch oracle (oracle/lpips_oracle.py): value and
gradient wrt the rendered image, shared seeded weights; PARITY UNPINNED (the `lpips` package and its weights are absent).  And the
pooling and image kernels of csrc/lpips.hip one by one (the pooling of a split map: tests/test_lpips_split_gpu.py)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import lpips_split_ref as R  # noqa: E402
from oracle import lpips_oracle as LO  # noqa: E402

pytestmark = pytest.mark.gpu
H16 = torch.float16


@pytest.mark.parametrize("H,W", [(64, 96), (50, 70), (136, 240)])
def test_lpips_value_and_gradient_vs_oracle(gpu, H, W, measurements):
    from syn3r_amd.gs.lpips import LPIPS
    m = LPIPS().init_random(gpu, seed=3)
    sd = R.seeded_state_dict(m.parameter_shapes(), seed=3)    # the same draws as init_random
    a, b = R.images(H, W, H)
    pred = a.to(gpu).requires_grad_(True)
    target = b.to(gpu)
    loss = m(pred, target)
    (3.0 * loss).backward()
    ao = a.double().requires_grad_(True)
    ref = LO.lpips(ao, b.double(), sd)
    (3.0 * ref).backward()
    gh, go = pred.grad.double().cpu(), ao.grad
    rel = float((gh - go).norm() / go.norm())
    cos = float((gh * go).sum() / (gh.norm() * go.norm()))
    measurements(f"lpips:{H}x{W}", value_rel=abs(float(loss) - float(ref)) / abs(float(ref)), grad_rel=rel, grad_cos=cos)
    # measured (round 5, gpurun_out/test_measurements.jsonl): value 9e-7 .. 2.5e-5 relative, gradient 5.4-5.7e-2 relative, cosine
    # 0.9983-0.9986 (the gradient's error is the 13 fp16 backward-data convolutions, profiles/r04/lpips_layers.txt)
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-4 * abs(float(ref.detach())), (float(loss.detach()), float(ref.detach()))
    # The gradient bar is NOT the suite's "2x the measurement" rule, on purpose: 2 x 5.7e-2 would accept a gradient that is 11 % off, i.e.
    # say nothing.  The error is the fp16 rounding of the 13 backward-data convolutions' activations and gradients against a float64
    # chain (per-layer table: profiles/r04/lpips_layers.txt); the bars sit ~5 % above the worst recorded value (5.7e-2, cosine 0.9983),
    # so a change of accumulation order may trip them - re-measure (gpurun_out/test_measurements.jsonl) before moving them, and the LPIPS
    # weights are unpinned anyway.
    assert rel < 6e-2 and cos > 0.998, (rel, cos)              # fp16 activations / gradients against float64
    # a second call with the same target object reuses its cached features and gives the same number
    assert float(m(pred.detach(), target)) == float(loss)
    assert float(m(target, target)) < 1e-6 * abs(float(ref)) + 1e-9


def test_lpips_state_dict_names_and_errors(gpu):
    from syn3r_amd import _lib as L
    from syn3r_amd.gs.lpips import LPIPS
    m = LPIPS()
    names = m.parameter_shapes()
    assert names["net.slice1.0.weight"] == (64, 3, 3, 3) and names["net.slice5.28.bias"] == (512,) and names["lin3.model.1.weight"] == (1, 512, 1, 1)
    assert len(names) == 26 + 5
    with pytest.raises(L.Syn3rError):
        m(torch.zeros(3, 32, 32, device=gpu), torch.zeros(3, 32, 32, device=gpu))           # weights not loaded
    m.init_random(gpu)
    with pytest.raises(ValueError):
        m(torch.zeros(3, 8, 8, device=gpu), torch.zeros(3, 8, 8, device=gpu))               # too small for four poolings
    with pytest.raises(KeyError):
        LPIPS().load_state_dict({"net.slice1.0.weight": torch.zeros(64, 3, 3, 3)}, gpu)


def test_trainer_uses_lpips_when_switched_on(gpu, tmp_path):
    """`opt.use_lpips_loss` (raised by DiffusionGS.run around refine_GS) x `opt.lpips_weight`: the term enters train_step and
    evaluate() reports the metric; off -> the loss is the photometric one alone."""
    tr, cam = R.trainer_with_lpips(gpu, "fp16")
    base = float(tr.train_step(cam))
    tr.opt.use_lpips_loss = True
    with_term = float(tr.train_step(cam))
    assert with_term > base * 1.02                            # the perceptual term is in the loss
    ev = tr.evaluate([cam])
    assert np.isfinite(ev["lpips"]) and ev["lpips"] > 0
    tr.lpips = None
    assert np.isnan(tr.evaluate([cam])["lpips"])


@pytest.mark.gpu
def test_lpips_layer_backward_saturates_instead_of_overflowing(gpu):
    """the layer backward multiplies by 1 / |a| and by the loss scale (~2.6e5 at relu5_3): a pixel whose feature norm
    is tiny but positive used to overflow the fp16 gradient to inf, which the backward convolutions then spread into the image
    gradient and Adam.  The kernel clamps to the fp16 range: every gradient is finite, the ordinary pixels are untouched."""
    from syn3r_amd import _lib as L
    lib = L.load()
    P, C = 256, 512
    g = torch.Generator().manual_seed(5)
    a = torch.rand(P, C, generator=g).to(torch.float16).to(gpu)
    b = torch.rand(P, C, generator=g).to(torch.float16).to(gpu)
    a[::16] = 0.0
    a[::16, 3] = 6e-5                                   # tiny but positive norm: 1 / |a| ~ 1.7e4
    a[8::16] = 0.0                                      # an all-zero pixel (norm 0 + 1e-10)
    w = torch.rand(C, generator=g).to(gpu)
    grad = torch.empty(P, C, dtype=torch.float16, device=gpu)
    L.check(lib.syn3r_lpips_layer_bwd_f16(L.ptr(a), L.ptr(b), L.ptr(w), P, C, 2.6e5, 0, L.ptr(grad), L.stream_ptr(gpu)), "lpips_layer_bwd")
    torch.cuda.synchronize()
    gf = grad.float()
    assert bool(torch.isfinite(gf).all())
    assert float(gf.abs().max()) <= 65504.0
    ordinary = gf[1::16].clone()
    assert float(ordinary.abs().max()) > 0.0
    # the same call at a scale no fp16 gradient survives: saturated at the largest finite fp16, never inf / NaN
    L.check(lib.syn3r_lpips_layer_bwd_f16(L.ptr(a), L.ptr(b), L.ptr(w), P, C, 1.0e12, 0, L.ptr(grad), L.stream_ptr(gpu)), "lpips_layer_bwd")
    torch.cuda.synchronize()
    gf = grad.float()
    assert bool(torch.isfinite(gf).all()) and float(gf.abs().max()) == 65504.0


@pytest.mark.parametrize("H,W,C", [(9, 14, 64), (5, 3, 8)])
def test_maxpool_and_backward_exact_with_ties(gpu, H, W, C):
    """syn3r_maxpool2_f16 / syn3r_maxpool2_bwd_f16 per element against torch on values of the quarter grid (fp16 and fp32 hold them
    exactly, ties are common): the odd last row / column is dropped by the forward and zeroed by the backward, the gradient of a
    tied window goes to its first cell, and the backward writes every cell (gx enters as 7).  5 x 3 x 8: one 8-channel chunk."""
    from syn3r_amd import _lib as L
    lib = L.load()
    Ho, Wo = H // 2, W // 2
    g = torch.Generator().manual_seed(12)                 # (a seed at which the 16 windows of the small case have their share of ties too)
    v = torch.randint(0, 6, (H, W, C), generator=g).float() * 0.25
    win = v[:2 * Ho, :2 * Wo].reshape(Ho, 2, Wo, 2, C)
    n_max = (win.amax(dim=(1, 3), keepdim=True) == win).sum(dim=(1, 3)).float()
    assert float(n_max.max()) >= 2 and float(n_max.mean()) > 1.25                # tied windows exist and are common
    x = v.reshape(-1, C).half().to(gpu)
    y = torch.full((Ho * Wo, C), 7.0, dtype=H16, device=gpu)
    L.check(lib.syn3r_maxpool2_f16(L.ptr(x), H, W, C, L.ptr(y), L.stream_ptr(gpu)), "maxpool2")
    vt = v.permute(2, 0, 1)[None].clone().requires_grad_(True)                   # [1, C, H, W] fp32
    ref = torch.nn.functional.max_pool2d(vt, 2, 2)
    assert torch.equal(y.cpu().float().reshape(Ho, Wo, C).permute(2, 0, 1)[None], ref.detach())
    gy = torch.randn(Ho * Wo, C, generator=g).half()
    ref.backward(gy.float().reshape(Ho, Wo, C).permute(2, 0, 1)[None])
    gx, gyd = torch.full((H * W, C), 7.0, dtype=H16, device=gpu), gy.to(gpu)
    L.check(lib.syn3r_maxpool2_bwd_f16(L.ptr(x), L.ptr(gyd), H, W, C, L.ptr(gx), L.stream_ptr(gpu)), "maxpool2_bwd")
    assert torch.equal(gx.cpu().float().reshape(H, W, C), vt.grad[0].permute(1, 2, 0))


@pytest.mark.parametrize("H,W", [(5, 7), (16, 16)])
def test_image_kernels_zero_fill_and_pair_value(gpu, H, W, measurements):
    """syn3r_lpips_image_f16 / syn3r_lpips_image_split_f16 on a uniform random image that holds the pixels 0 and 1 (5 x 7: two
    blocks, the second partial).  The padding channels are exactly zero (the outputs enter as 7), the hi plane of the split entry
    is the plain entry's output, and the pair float(hi) + float(lo) lies within 2^-20 absolute of ((2x - 1) - shift) / scale in
    float64 on the fp32-rounded constants: three fp32 operations on |f| < 2.7 give at most ~2^-21, the fp16 rounding of a remainder
    of at most 2^-9.5 at most 2^-20.5 - under 2^-19.5 together; a float32 / float16 emulation of the kernel's arithmetic on 2M
    pixels reaches 2^-20.96 at worst, the bar is twice that."""
    from syn3r_amd import _lib as L
    lib = L.load()
    img = torch.rand(3, H, W, generator=torch.Generator().manual_seed(13))
    img[:, 0, 0], img[:, 0, 1] = 0.0, 1.0
    x = img.to(gpu)
    plain = torch.full((H * W, 64), 7.0, dtype=H16, device=gpu)
    split = torch.full((H * W, 64), 7.0, dtype=H16, device=gpu)
    L.check(lib.syn3r_lpips_image_f16(L.ptr(x), H, W, L.ptr(plain), L.stream_ptr(gpu)), "lpips_image")
    L.check(lib.syn3r_lpips_image_split_f16(L.ptr(x), H, W, L.ptr(split), L.stream_ptr(gpu)), "lpips_image_split")
    p, s = plain.cpu(), split.cpu()
    assert bool((p[:, 3:] == 0).all())
    assert bool((s[:, 6:] == 0).all()) and torch.equal(s[:, :3], p[:, :3])
    ref = ((2 * img.double()[None] - 1) - LO.SHIFT.double()) / LO.SCALE.double()          # fp32 constants, as the kernel's
    err = float((s[:, :3].double() + s[:, 3:6].double() - ref[0].reshape(3, H * W).T).abs().max())
    measurements(f"lpips:image_pair:{H}x{W}", max_abs=err)
    print(f"lpips image pair {H}x{W}: max abs error {err:.3e} (2^{np.log2(max(err, 1e-300)):.2f})")
    assert err <= 2.0 ** -20, err
