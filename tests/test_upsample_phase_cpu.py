"""The fold behind the four-phase upsampling convolution (include/syn3r_hip.h: syn3r_pack_upsample4_f16), without a GPU:
the identity itself in float64, the two implementations of the fold rule bit for bit, and what the one extra fp16 rounding of
the folded weights costs against the 9-tap form."""
import ctypes

import pytest
import torch

from upsample_phase_ref import GPU_SHAPES, H, fold, four_phase, gpu_case, nine_tap, rnd


@pytest.mark.parametrize("NB,Hi,Wi", [(2, 5, 7), (1, 1, 1), (1, 2, 1), (3, 8, 12)])
def test_fold_identity_float64(NB, Hi, Wi):
    """conv2d(interpolate(x, 2, 'nearest'), w, padding=1) == the four 2x2 phase convolutions on the summed taps, borders included
    (the padding of the upsampled image falls on input row / column -1 or Hi / Wi).  Float64 on both sides: what is left is
    the reassociation of <= 9 Cin products of O(1) numbers, far below 1e-12."""
    g = torch.Generator().manual_seed(NB * 100 + Hi * 10 + Wi)
    Cin, Cout = 6, 5
    x = torch.randn(NB, Hi, Wi, Cin, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, 3, 3, Cin, generator=g, dtype=torch.float64)
    b = torch.randn(Cout, generator=g, dtype=torch.float64)
    ref = nine_tap(x, w, b)
    got = four_phase(x, fold(w), b)
    assert got.shape == ref.shape == (NB, 2 * Hi, 2 * Wi, Cout)
    err = (got - ref).abs().max().item()
    print(f"fold identity {NB}x{Hi}x{Wi}: max |diff| = {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("Cin", [16, 192])
def test_python_pack_equals_host_pack_bitwise(Cin):
    """ops.pack_upsample4 (torch) and syn3r_pack_upsample4_f16 (plain host C++, what the native executor calls) are one rule:
    fp32 sums in ascending (ty, tx) order, one rounding to fp16."""
    from syn3r_amd import _lib
    from syn3r_amd.unet import ops
    lib = _lib.load()
    Cout = 40
    g = torch.Generator().manual_seed(Cin)
    w = rnd(g, Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5)
    w[0, 0, 0, 0], w[1, 1, 1, 1], w[2, 2, 2, 2] = 65504.0, 6.0e-8, -0.0           # fp16 edges: largest, a subnormal, minus zero
    w[3, 1, :, 3], w[4, :, 1, 4] = 40000.0, 40000.0                               # sums that overflow fp16 (inf on both sides)
    want = ops.pack_upsample4(w)
    got = torch.empty((4, Cout, 2, 2, Cin), dtype=H)
    rc = lib.syn3r_pack_upsample4_f16(ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(got.data_ptr()), Cout, Cin)
    assert rc == 0, lib.syn3r_last_error()
    assert want.shape == got.shape
    assert torch.equal(want.view(torch.int16), got.view(torch.int16))
    # and it is the rule of the float64 restatement, rounded once
    assert torch.equal(want[torch.isfinite(want)], fold(w.float()).to(H)[torch.isfinite(want)])
    assert lib.syn3r_pack_upsample4_f16(None, None, Cout, Cin) != 0 and b"null" in lib.syn3r_last_error()


def test_fp16_fold_parity_budget():
    """What rounding the SUMMED weights to fp16 costs against the 9-tap form on the same fp16 weights, at a UNet-like
    convolution (Cin = 320, weights of scale (9 Cin)^-0.5), both evaluated in float64.  A folded weight carries one extra
    rounding of relative size <= 2^-11 (none where it is a single tap), the errors of different weights are independent, so
    the relative rms of the output difference is below 2^-11 = 4.9e-4: half an fp16 step of the output.  Measured: 2.1e-4."""
    g = torch.Generator().manual_seed(320)
    NB, Hi, Wi, Cin, Cout = 1, 6, 8, 320, 64
    x = rnd(g, NB, Hi, Wi, Cin)
    w = rnd(g, Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5)
    ref = nine_tap(x, w)
    got = four_phase(x, fold(w.float()).to(H))
    rel_rms = ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    print(f"fp16 fold parity, Cin = {Cin}: relative rms {rel_rms:.3e}, max |diff| {(got - ref).abs().max().item():.3e}")
    assert rel_rms <= 2.0 ** -11


@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_folded_fp16_weights_stay_inside_the_gpu_bar(shape):
    """The GPU test compares the phase kernel with the 9-tap kernel at 2e-3 of the largest output; the fold's own share of
    that (float64 on both sides, so without any kernel) has to stay inside it at the four shapes it uses."""
    c = gpu_case(*shape)
    err = (c["ref4"] - c["ref9"]).abs().max().item()
    bar = 2e-3 * c["ref9"].abs().max().item()
    print(f"{shape}: fold |diff| max {err:.3e}, bar {bar:.3e}")
    assert err <= bar
