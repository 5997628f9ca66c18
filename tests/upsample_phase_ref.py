"""The four-phase form of `nearest-2x upsample + 3x3 convolution` (include/syn3r_hip.h: syn3r_pack_upsample4_f16 /
syn3r_conv2d3x3_up4_f16) restated in float64 torch, for tests/test_upsample_phase_cpu.py and tests/test_upsample_phase_gpu.py.
A plain module, not a conftest.

After the upsample the 3x3 window of output pixel (2i + py, 2j + px) covers input pixels (i + py - 1 + a, j + px - 1 + b),
a, b in {0, 1}; filter rows ty fall on block row a as  py = 0: {0} | {1, 2},  py = 1: {0, 1} | {2}  (columns the same with px)."""
import functools

import torch
import torch.nn.functional as Fn

H = torch.float16
GROUPS = (((0,), (1, 2)), ((0, 1), (2,)))

# the GPU cases of the issue: (NB, Hi, Wi, Cin, Cout)
GPU_SHAPES = [(3, 5, 7, 64, 40), (2, 8, 12, 192, 320), (5, 9, 16, 64, 640), (2, 16, 32, 128, 320)]


def fold(w: torch.Tensor) -> torch.Tensor:
    """[Cout,3,3,Cin] -> [4,Cout,2,2,Cin] in the dtype of `w`, taps summed in ascending (ty, tx) order (no rounding other than
    that dtype's additions: exact for the float64 identity check)."""
    out = w.new_zeros((4, w.shape[0], 2, 2, w.shape[3]))
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    for ty in GROUPS[py][a]:
                        for tx in GROUPS[px][b]:
                            out[2 * py + px, :, a, b] += w[:, ty, tx]
    return out


def nine_tap(x: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """x [NB,Hi,Wi,Cin], w [Cout,3,3,Cin] (OHWI) -> [NB,2Hi,2Wi,Cout] in float64: conv2d(interpolate(x, 2, 'nearest'), w, padding=1)."""
    xin = Fn.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    y = Fn.conv2d(xin, w.double().permute(0, 3, 1, 2), None if bias is None else bias.double(), padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


def four_phase(x: torch.Tensor, w4: torch.Tensor, bias=None) -> torch.Tensor:
    """x [NB,Hi,Wi,Cin], w4 [4,Cout,2,2,Cin] -> [NB,2Hi,2Wi,Cout] in float64: four 2x2 convolutions at input resolution."""
    NB, Hi, Wi, Cin = x.shape
    xp = Fn.pad(x.double(), (0, 0, 1, 1, 1, 1))                      # one zero row / column on every side
    w4 = w4.double()
    out = torch.zeros((NB, 2 * Hi, 2 * Wi, w4.shape[1]), dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            acc = torch.zeros((NB, Hi, Wi, w4.shape[1]), dtype=torch.float64)
            for a in range(2):
                for b in range(2):
                    # input pixel (i + py - 1 + a, j + px - 1 + b) = padded pixel (i + py + a, j + px + b)
                    acc += torch.einsum("nhwc,oc->nhwo", xp[:, py + a:py + a + Hi, px + b:px + b + Wi], w4[2 * py + px, :, a, b])
            out[:, py::2, px::2] = acc
    if bias is not None:
        out += bias.double()
    return out


def rnd(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(H)


@functools.lru_cache(maxsize=None)
def gpu_case(NB, Hi, Wi, Cin, Cout):
    """Inputs (fp16, host) and the two float64 references of one GPU case, computed once per process and never modified:
    x, w (OHWI), bias, w4 (the fold rule in torch: fp32 sums, one rounding), ref4 (four-phase form of the fp16 w4), ref9 (9-tap)."""
    g = torch.Generator().manual_seed(1000 * NB + 10 * Hi + Cout)
    x = rnd(g, NB, Hi, Wi, Cin)
    w = rnd(g, Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5)
    b = rnd(g, Cout)
    w4 = fold(w.float()).to(H)
    return dict(x=x, w=w, b=b, w4=w4, ref4=four_phase(x, w4, b), ref9=nine_tap(x, w, b))
