"""LPIPS(precision="fp16x2") on the HIP path: every forward activation stored as an fp16 pair hi + lo (csrc/lpips.hip, the split
epilogue of the implicit-GEMM convolution).  Same sizes, seeds and oracle call as tests/test_lpips_gpu.py; the kernels of the mode
one by one; one trainer step."""
import math
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


def _split(v):
    """fp32 [P, C] -> the pair tensor [P, 2C] fp16 (hi plane | lo plane)."""
    hi = v.half()
    lo = (v - hi.float()).half()
    return torch.cat([hi, lo], dim=1).contiguous()


def _join(t):
    C = t.shape[1] // 2
    return t[:, :C].float() + t[:, C:].float()


@pytest.mark.parametrize("H,W", [(64, 96), (50, 70), (136, 240)])
def test_lpips_split_value_and_gradient_vs_oracle(gpu, H, W, measurements):
    """Bars: value 1e-4 relative (the fp16 mode's); gradient rel < 1e-3 and cos > 1 - 1e-6 against float64 - ~2.3x the 4.3-4.5e-4
    that the float64 emulation with fp16 pairs and fp16 scaled gradients gives (tests/test_lpips_split_cpu.py), the suite's 2x
    rule; torch fp32 itself scatters 2.7e-6 .. 1.5e-4 across these sizes.  The fp16 mode sits at 5.4-5.75e-2.
    Measured on an MI355X: value 2.6e-8 .. 1.4e-7, gradient 5.04e-4 / 5.14e-4 / 8.65e-4 (64x96 / 50x70 / 136x240), 1 - cos 1.3e-7 ..
    3.7e-7.  136x240 lies at twice its emulation, 13 % under the bar.  Layer by layer (profiles/r07/lpips_layers_fp16x2.txt) relu2_2,
    relu3_3 and relu4_3 agree with the emulation to three digits; relu1_2 (9.5e-4 for 2.5e-4) and relu5_3 (1.8e-3 for 7.3e-4) carry
    the whole gap, the default mode has the same excess at relu1_2, and the emulation rules out saturation, subnormal gradients and
    fp32 arithmetic.  The excess sits in code both modes share, on the paths only those two layers take."""
    from syn3r_amd.gs.lpips import LPIPS
    m = LPIPS(precision="fp16x2").init_random(gpu, seed=3)
    sd = R.seeded_state_dict(m.parameter_shapes(), seed=3)
    a, b = R.images(H, W, H)
    pred = a.to(gpu).requires_grad_(True)
    target = b.to(gpu)
    loss = m(pred, target)
    (3.0 * loss).backward()
    ao = a.double().requires_grad_(True)
    ref = LO.lpips(ao, b.double(), sd)
    (3.0 * ref).backward()
    rel, cos = R.grad_error(pred.grad.double().cpu(), ao.grad)
    value_rel = abs(float(loss.detach()) - float(ref.detach())) / abs(float(ref.detach()))
    measurements(f"lpips_split:{H}x{W}", value_rel=value_rel, grad_rel=rel, grad_cos=cos)
    print(f"lpips fp16x2 {H}x{W}: value_rel {value_rel:.3e} grad_rel {rel:.3e} 1-cos {1 - cos:.3e}")
    loss, ref = loss.detach(), ref.detach()
    assert value_rel < 1e-4, (float(loss), float(ref))
    assert rel < 1e-3 and cos > 1 - 1e-6, (rel, cos)
    # the cache: a second call with the same target object reuses its features and gives the same number
    n_cached = len(m._target_cache)
    assert float(m(pred.detach(), target)) == float(loss) and len(m._target_cache) == n_cached
    assert float(m(target, target)) < 1e-6 * abs(float(ref)) + 1e-9
    # a default-mode model on the same target OBJECT keeps features of its own (another layout: [P, C] against [P, 2C])
    m16 = LPIPS().init_random(gpu, seed=3)
    l16 = float(m16(pred.detach(), target))
    assert abs(l16 - float(ref)) < 1e-4 * abs(float(ref))
    k16, k32 = next(iter(m16._target_cache)), next(iter(m._target_cache))
    assert k16[0] == k32[0] == id(target) and k16 != k32
    f16, f32 = m16._target_cache[k16][2], m._target_cache[k32][2]
    assert all(x.shape[1] * 2 == y.shape[1] and x.data_ptr() != y.data_ptr() for x, y in zip(f16, f32))
    assert float(m(pred.detach(), target)) == float(loss)


def test_split_maxpool_and_backward_with_ties_in_hi(gpu):
    """The 2x2 pooling of a split map compares float(hi) + float(lo): windows whose hi planes tie are decided by lo, windows whose
    sums tie go to the first cell (torch's rule), odd last row / column dropped; the backward routes the gradient the same way."""
    from syn3r_amd import _lib as L
    lib = L.load()
    Hh, Ww, C = 9, 14, 64
    g = torch.Generator().manual_seed(11)
    hi = (torch.randint(0, 6, (Hh, Ww, C), generator=g).float() * 0.25).half()          # few distinct values: many ties in hi
    lo = (torch.randint(-2, 3, (Hh, Ww, C), generator=g).float() * 2.0 ** -14).half()   # far below hi's spacing, five values: exact ties too
    v = hi.float() + lo.float()
    win = v[:8, :14].reshape(4, 2, 7, 2, C)
    assert float((win.amax(dim=(1, 3), keepdim=True) == win).sum(dim=(1, 3)).float().max()) >= 2      # exact ties in the sum exist
    hwin = hi[:8, :14].float().reshape(4, 2, 7, 2, C)
    assert float((hwin.amax(dim=(1, 3), keepdim=True) == hwin).sum(dim=(1, 3)).float().mean()) > 1.25  # and ties in hi are common
    x = torch.cat([hi.reshape(-1, C), lo.reshape(-1, C)], dim=1).contiguous().to(gpu)
    y = torch.empty((Hh // 2) * (Ww // 2), 2 * C, dtype=H16, device=gpu)
    L.check(lib.syn3r_maxpool2_split_f16(L.ptr(x), Hh, Ww, C, L.ptr(y), L.stream_ptr(gpu)), "maxpool2_split")
    vt = v.permute(2, 0, 1)[None].clone().requires_grad_(True)                          # [1, C, H, W] fp32: the pair sums are exact
    ref = torch.nn.functional.max_pool2d(vt, 2, 2)
    got = _join(y.cpu()).reshape(Hh // 2, Ww // 2, C).permute(2, 0, 1)[None]
    assert torch.equal(got, ref.detach())
    # the winning PAIR is copied, not a re-split of the sum
    yh = y.cpu()[:, :C].float().reshape(Hh // 2, Ww // 2, C)
    assert bool((yh == hwin.amax(dim=(1, 3))).all())
    gy = torch.randn((Hh // 2) * (Ww // 2), C, generator=g).half()
    ref.backward(gy.float().reshape(Hh // 2, Ww // 2, C).permute(2, 0, 1)[None])
    gx = torch.full((Hh * Ww, C), 7.0, dtype=H16, device=gpu)
    L.check(lib.syn3r_maxpool2_bwd_split_f16(L.ptr(x), L.ptr(gy.to(gpu)), Hh, Ww, C, L.ptr(gx), L.stream_ptr(gpu)), "maxpool2_bwd_split")
    assert torch.equal(gx.cpu().float().reshape(Hh, Ww, C), vt.grad[0].permute(1, 2, 0))


def _conv_case(gpu, Hh, Ww, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.relu(torch.randn(Hh * Ww, Cin, generator=g))                     # a post-ReLU map, O(1)
    x = _split(v)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * math.sqrt(2.0 / (Cin * 9))).half()
    b = (0.05 * torch.randn(Cout, generator=g)).half()
    xin = _join(x).double().reshape(Hh, Ww, Cin).permute(2, 0, 1)[None]
    ref = torch.relu(torch.nn.functional.conv2d(xin, w.double(), b.double(), padding=1))[0].permute(1, 2, 0).reshape(Hh * Ww, Cout)
    wf = w.permute(0, 2, 3, 1)
    return x.to(gpu), torch.cat([wf, wf], dim=3).contiguous().to(gpu), b.to(gpu), ref


def _epilogue_errors(gpu):
    from syn3r_amd.gs.lpips import _conv, _conv_split
    Hh, Ww, Cin, Cout = 40, 56, 64, 128
    x, w2, b, ref = _conv_case(gpu, Hh, Ww, Cin, Cout, seed=21)
    out = _conv_split(x, w2, b, Hh, Ww, relu=True, split_out=True)
    plain = _conv(x, w2, b, Hh, Ww, relu=True)          # the fp16 entry on the same operands: half(v) of the same accumulator
    torch.cuda.synchronize()
    o = out.cpu()
    return o[:, :Cout], o[:, Cout:], plain.cpu(), ref


def test_split_epilogue_planes(gpu, measurements):
    """One 64 -> 128 layer on a split input.  The hi plane is bit for bit what the fp16 entry stores for the same operands (same
    kernel body, same accumulation order: hi = half(v)); lo is a rounding remainder of hi and nothing more; and the pair IS more
    than hi: the median relative error against the float64 convolution is that of an fp32 accumulation of 576 products
    (~sqrt(576) 2^-24 = 2^-19.4 of the partial sums), where one fp16 has ~2^-13 - the bar 2^-17 lies between the two."""
    hi, lo, plain, ref = _epilogue_errors(gpu)
    assert torch.equal(hi, plain)
    hi, lo = hi.float(), lo.float()
    got = (hi + lo).double()
    assert bool(torch.isfinite(got).all())
    assert bool((lo.abs() <= hi.abs() * 2.0 ** -11 + 2.0 ** -25).all())
    assert float(((ref == 0) == (got == 0)).float().mean()) > 0.9999          # the ReLU zeros agree (but for sums within rounding of 0)
    big = ref > 1e-3
    med_pair = float(((got - ref).abs() / ref.clamp_min(1e-30))[big].median())
    med_hi = float(((hi.double() - ref).abs() / ref.clamp_min(1e-30))[big].median())
    measurements("lpips_split:epilogue_planes", median_rel_pair=med_pair, median_rel_hi_alone=med_hi)
    print(f"split epilogue 64->128: median relative error of the pair {med_pair:.3e}, of hi alone {med_hi:.3e}")
    assert med_pair < 2.0 ** -17 < med_hi


def _exact_conv_case(seed):
    """Operands of a 64 -> 128 layer on binary grids, so that fp32 sums them without a rounding: the map 0 (half of it, as after a
    ReLU) or a multiple of 2^-10 below 4 - 12 bits, so a quarter of the non-zero values has a lo of +-2^-10; weights -6..6 times
    2^-7; bias a multiple of 2^-17 below 2^-6.  Every product and the bias are multiples of 2^-17."""
    Hh, Ww, Cin, Cout = 40, 56, 64, 128
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, 4096, (Hh * Ww, Cin), generator=g).float() * 2.0 ** -10
    v = v * (torch.rand(Hh * Ww, Cin, generator=g) < 0.5)
    w = (torch.randint(-6, 7, (Cout, Cin, 3, 3), generator=g).float() * 2.0 ** -7).half()
    b = (torch.randint(-2047, 2048, (Cout,), generator=g).float() * 2.0 ** -17).half()
    return Hh, Ww, Cin, Cout, _split(v), w, b


def test_split_epilogue_against_float64_convolution(gpu, measurements):
    """The issue's bar: on one 64 -> 128 layer, recombined hi + lo within 2^-20 relative of the fp32 result for values above 1e-3,
    against a float64 convolution.

    "The fp32 result" is the kernel's accumulator v after bias and ReLU, which no entry returns.  A float64 convolution of random
    operands is not it: fp32 rounds each of the 1152 additions at 2^-24 of partial sums that are O(1), and a result of 1e-3 left
    after cancellation carries that as ~2e-4 relative, in any fp32 convolution (with the operands of test_split_epilogue_planes
    7.5 % of the values above 1e-3 lie beyond 2^-20 of the float64 sum for that reason, median 2^-22.4).  So the operands here are
    ones that fp32 sums exactly in any order: all products and the bias are multiples of 2^-17, and the sum of their magnitudes,
    which bounds every partial sum of every grouping (k-tiles, MFMA blocks, hi and lo halves), stays below 2^5 - 22 bits, asserted
    below.  The float64 convolution then IS the fp32 accumulator, bit for bit, and what the test measures is the epilogue:
    hi = half(v), lo = half(v - float(hi)), both planes at their place.  The results, multiples of 2^-17 up to ~6, need up to 20
    bits; those between 1e-3 and 2^-5 have a lo below fp16's normal range.

    What the format cannot do, and this test does not claim: lo is an fp16 number with a spacing of 2^-24 below 2^-14, so the pair
    holds an ARBITRARY fp32 v to 2^-25 absolute - ">= 21 significant bits" from v = 2^-5 up, fewer below (profiles/README.md, "LPIPS gradient error")."""
    from syn3r_amd.gs.lpips import _conv_split
    Hh, Ww, Cin, Cout, x, w, b = _exact_conv_case(seed=23)
    assert float(x[:, Cin:].abs().max()) == 2.0 ** -10 and 0.05 < float((x[:, Cin:] != 0).float().mean()) < 0.2   # the lo plane is in use
    nchw = lambda t: t.double().reshape(Hh, Ww, Cin).permute(2, 0, 1)[None]
    xin = nchw(x[:, :Cin]) + nchw(x[:, Cin:])
    pre = torch.nn.functional.conv2d(xin, w.double(), b.double(), padding=1)
    ref = torch.relu(pre)[0].permute(1, 2, 0).reshape(Hh * Ww, Cout)
    mag = torch.nn.functional.conv2d(nchw(x[:, :Cin]).abs() + nchw(x[:, Cin:]).abs(), w.double().abs(), b.double().abs(), padding=1)
    assert float(mag.max()) < 2.0 ** 5                                         # every partial sum: a multiple of 2^-17 below 2^5
    assert torch.equal(ref.float().double(), ref)                              # and so is the result: fp32 holds it exactly
    wf = w.permute(0, 2, 3, 1)
    out = _conv_split(x.to(gpu), torch.cat([wf, wf], dim=3).contiguous().to(gpu), b.to(gpu), Hh, Ww, relu=True, split_out=True)
    torch.cuda.synchronize()
    o = out.cpu()
    hi, lo = o[:, :Cout].float(), o[:, Cout:].float()
    got = (hi + lo).double()
    big = ref > 1e-3
    small_lo = big & (ref < 2.0 ** -5)
    assert int(big.sum()) > 0.4 * ref.numel() and int(small_lo.sum()) > 1000 and float(ref.max()) > 4.0
    assert float((lo[big] != 0).float().mean()) > 0.5                          # most results do not fit one fp16
    err = ((got - ref).abs() / ref.clamp_min(1e-30))[big]
    err_hi = ((hi.double() - ref).abs() / ref.clamp_min(1e-30))[big]
    inexact = float((err > 0).float().mean())
    measurements("lpips_split:epilogue_64_128", max_rel=float(err.max()), share_inexact=inexact, max_rel_hi_alone=float(err_hi.max()),
                 max_abs_of_small=float((got - ref).abs()[~big].max()))
    print(f"split epilogue 64->128, exactly summable operands: max rel (values > 1e-3) {float(err.max()):.3e}, share not exact {inexact:.3e}, "
          f"hi alone {float(err_hi.max()):.3e}, max abs at or below 1e-3 {float((got - ref).abs()[~big].max()):.3e}")
    assert float(err.max()) <= 2.0 ** -20, (float(err.max()), inexact)
    assert torch.equal(got[~big], ref[~big])                                   # the zeros of the ReLU and the few values up to 1e-3


def test_split_backward_data_convolution_masks_by_the_hi_plane(gpu):
    """split_out = 0 with a mask: the plain fp16 backward-data result, zeroed where the hi plane of a split map [P, 2 Cin] is <= 0
    (row stride 2 Cin) - against the fp16 entry with the hi plane copied out as a dense mask: bit-identical."""
    from syn3r_amd.gs.lpips import _conv, _conv_split
    Hh, Ww, Cin, Cout = 24, 40, 128, 64
    g = torch.Generator().manual_seed(31)
    grad = torch.randn(Hh * Ww, Cout, generator=g).half().to(gpu)
    wb = (torch.randn(Cin, 3, 3, Cout, generator=g) * 0.05).half().to(gpu)
    below = _split(torch.relu(torch.randn(Hh * Ww, Cin, generator=g))).to(gpu)
    got = _conv_split(grad, wb, None, Hh, Ww, relu=False, split_out=False, mask=below)
    ref = _conv(grad, wb, None, Hh, Ww, relu=False, mask=below[:, :Cin].contiguous())
    assert got.shape == (Hh * Ww, Cin) and torch.equal(got, ref)
    assert 0.3 < float((got == 0).float().mean()) < 0.7


def test_trainer_step_with_split_lpips(gpu):
    """One GSTrainer.train_step with a split-mode LPIPS attached: finite loss, the term is in it, the parameters move."""
    tr, cam = R.trainer_with_lpips(gpu, "fp16x2")
    base = float(tr.train_step(cam))
    tr.opt.use_lpips_loss = True
    before = tr.gaussians.get_xyz.detach().clone()
    with_term = float(tr.train_step(cam))
    assert np.isfinite(with_term) and with_term > base * 1.02
    after = tr.gaussians.get_xyz.detach()
    assert bool(torch.isfinite(after).all()) and float((after - before).abs().max()) > 0
