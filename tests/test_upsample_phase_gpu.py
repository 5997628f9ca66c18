"""syn3r_conv2d3x3_up4_f16 (k_gemm_z<conv2d, UP4>, csrc/gemm_z.h): nearest-2x upsample + 3x3 convolution as four 2x2 phase
convolutions on weights folded at load.  Reference semantics: upsampling.py:172-183.

The kernel is checked against a float64 four-phase reference built from the SAME folded fp16 weights (so the fold is not part of
what is measured), against the 9-tap kernel on the same inputs, for its GroupNorm partial sums, its refusals, and for writing every
output element.  Shapes: odd sizes with M4 = NB Hi Wi = 105 < one 256-row tile and rows of a tile straddling images; three
64-channel chunks per tap with one whole 320-column tile; M4 = 720 (a ragged last m-tile in every phase), Hi Wi % 32 != 0 and two
n-tiles; Hi Wi % 32 == 0 (partial sums on, four m-tiles per phase)."""
import ctypes
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from poison import poisoned  # noqa: E402
from upsample_phase_ref import GPU_SHAPES, H, gpu_case  # noqa: E402

pytestmark = pytest.mark.gpu


def close(a, b, tol=2e-3):           # the helper and bar of tests/test_unet_ops_gpu.py::test_conv3x3_upsample_every_kernel
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item() + 1e-6
    print(f"max err {err:.4e}, scale {ref:.4e}, bar {tol * ref + 1e-3:.4e}")
    assert err <= tol * ref + 1e-3, (err, ref)


def run_up4(c, gpu, gn_stats=False):
    from syn3r_amd.unet import ops
    w4 = ops.pack_upsample4(c["w"].to(gpu))
    assert torch.equal(w4.cpu(), c["w4"]), "the fold on the device differs from the fold on the host"
    return ops.conv3x3_up4(c["x"].to(gpu), w4, c["b"].to(gpu), gn_stats=gn_stats)


@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_kernel_against_float64_four_phase_reference(shape, gpu):
    c = gpu_case(*shape)
    out = run_up4(c, gpu)
    assert out.shape == c["ref4"].shape
    close(out.cpu(), c["ref4"])
    # per phase as well: a phase stored to another phase's pixels would still pass a max-norm check of a smooth enough output
    for py in range(2):
        for px in range(2):
            close(out.cpu()[:, py::2, px::2], c["ref4"][:, py::2, px::2])


@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_kernel_against_nine_tap_kernel(shape, gpu):
    from syn3r_amd.unet import ops
    c = gpu_case(*shape)
    out = run_up4(c, gpu)
    out9 = ops.conv3x3(c["x"].to(gpu), c["w"].to(gpu), c["b"].to(gpu), upsample=True)
    assert out.shape == out9.shape
    err = (out.float() - out9.float()).abs().max().item()
    bar = 2e-3 * c["ref9"].abs().max().item()
    print(f"{shape}: phase kernel against 9-tap kernel max |diff| {err:.4e}, bar {bar:.4e}")
    assert err <= bar


def expected_up4_partials(out: torch.Tensor) -> torch.Tensor:
    """[NB,2Hi,2Wi,N] fp16 -> [NB * 4 * Hi Wi / 32, 2, N/10] fp64 in the slot order of include/syn3r_hip.h: image, phase,
    32-pixel block of that phase's Hi x Wi pixels in row-major order."""
    NB, Ho, Wo, N = out.shape
    rows = []
    for n in range(NB):
        for py in range(2):
            for px in range(2):
                x = out[n, py::2, px::2].double().reshape(-1, 32, N // 10, 10)
                rows.append(torch.stack([x.sum((1, 3)), (x * x).sum((1, 3))], dim=1))
    return torch.cat(rows, 0)


def test_partials_and_groupnorm(gpu):
    """Hi Wi % 32 == 0: the epilogue leaves the GroupNorm partial sums; GroupNorm from them equals the statistics-pass form at
    the bar of tests/test_gn_epilogue_gpu.py (2e-3 of the largest output), twice bit for bit; asking changes no output bit."""
    from syn3r_amd.unet import ops
    shape = GPU_SHAPES[3]
    NB, Hi, Wi, Cin, Cout = shape
    c = gpu_case(*shape)
    plain = run_up4(c, gpu)
    out = run_up4(c, gpu, gn_stats=True)
    again = run_up4(c, gpu, gn_stats=True)
    part = getattr(out, "gn_part", None)
    assert part is not None, "the kernel did not write the partial sums"
    assert torch.equal(out, plain), "asking for the partial sums changed the output"
    assert torch.equal(part, again.gn_part) and torch.equal(out, again)
    exp = expected_up4_partials(out.cpu())
    got = part.cpu().view(NB * 4 * Hi * Wi // 32, 2, Cout // 10).double()
    assert (got[:, 0] - exp[:, 0]).abs().max().item() <= 2e-5 * (exp[:, 0].abs().max().item() + 32 * 10)       # (test_gn_epilogue_gpu.check_partials)
    assert (got[:, 1] - exp[:, 1]).abs().max().item() <= 2e-5 * (exp[:, 1].abs().max().item() + 1e-6)
    g = torch.Generator().manual_seed(7)
    ga, be = (torch.randn(Cout, generator=g)).to(H).to(gpu), (torch.randn(Cout, generator=g)).to(H).to(gpu)
    x2d = ops.keep_gn(out.view(-1, Cout), out)
    y = ops.groupnorm(x2d, ga, be, NB, 1e-5, True)
    y_stats = ops.groupnorm(x2d, ga, be, NB, 1e-5, True, use_partials=False)
    err = (y.float() - y_stats.float()).abs().max().item()
    bar = 2e-3 * (y_stats.float().abs().max().item() + 1e-6)
    print(f"GroupNorm from producer partials against the statistics pass: max |diff| {err:.4e}, bar {bar:.4e}")
    assert err <= bar
    assert torch.equal(y, ops.groupnorm(x2d, ga, be, NB, 1e-5, True))
    # Hi Wi % 32 != 0 (9 x 16 = 144 pixels per image and phase) reports "not written": GroupNorm runs its statistics pass
    c2 = gpu_case(*GPU_SHAPES[2])
    assert getattr(run_up4(c2, gpu, gn_stats=True), "gn_part", None) is None


def test_refusals(gpu):
    """Cin = 24 and a non-null residual are refused with a message, and nothing is launched (the output keeps its fill)."""
    from syn3r_amd import _lib
    lib = _lib.load()
    NB, Hi, Wi, Cout = 1, 4, 4, 16
    out = torch.full((NB, 2 * Hi, 2 * Wi, Cout), 3.0, dtype=H, device=gpu)
    res = torch.zeros_like(out)
    written = ctypes.c_int(7)

    def call(Cin, residual):
        x = torch.ones((NB, Hi, Wi, Cin), dtype=H, device=gpu)
        w4 = torch.ones((4, Cout, 2, 2, Cin), dtype=H, device=gpu)
        return lib.syn3r_conv2d3x3_up4_f16(x.data_ptr(), w4.data_ptr(), out.data_ptr(), None, residual, NB, Hi, Wi, Cin, Cout, None, 0,
                                           ctypes.byref(written), None)
    assert call(24, None) != 0 and b"Cin=24" in lib.syn3r_last_error() and written.value == 0
    written.value = 7
    assert call(64, res.data_ptr()) != 0 and b"residual" in lib.syn3r_last_error() and written.value == 0
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()), "a refused call wrote to the output"
    assert call(64, None) == 0
    torch.cuda.synchronize()
    # all-ones operands: 4 taps x 64 channels inside, 2 taps on an edge, 1 in a corner (the padding ring of the upsampled image)
    o = out[0, :, :, 0].float().cpu()
    assert bool((out.float() == out[..., :1].float()).all())
    assert bool((o[1:-1, 1:-1] == 256.0).all()) and bool((o[0, 1:-1] == 128.0).all()) and bool((o[1:-1, -1] == 128.0).all())
    assert o[0, 0] == o[0, -1] == o[-1, 0] == o[-1, -1] == 64.0


@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_every_output_element_is_written(shape, gpu, monkeypatch):
    """The output allocation pre-filled with NaN (tests/poison.py, pattern 0xFF): every element is written, ragged tiles and all
    four phases included, and the result does not depend on the fill."""
    c = gpu_case(*shape)
    base = run_up4(c, gpu, gn_stats=True)
    with poisoned(monkeypatch, 0xFF):
        out = run_up4(c, gpu, gn_stats=True)
        torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), f"{int((~torch.isfinite(out)).sum())} output elements were not written"
    assert torch.equal(out, base)
    if getattr(base, "gn_part", None) is not None:
        assert bool(torch.isfinite(out.gn_part).all()) and torch.equal(out.gn_part, base.gn_part)
