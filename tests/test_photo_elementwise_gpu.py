"""The fused photometric loss (csrc/photo_loss.hip: k_photo_fwd, k_photo_bwd, photo_final; with and without a weight map) per pixel and per
tile against float64.

The ABI entries are called directly with a workspace of the test's own, filled with the NaN pattern of tests/poison.py first, so the
three derivative maps and the per-tile sums the kernels leave there can be read.  References, derived slacks (GAMMA, GAMMA_B, DEPTH),
designs and the five checks come from tests/photo_ref.py; tests/test_photo_elementwise_cpu.py shows without a GPU that an fp32
restatement of both kernels meets the same checks on the same designs and that nine subtly wrong kernels do not.

  1 forward per pixel     each stored map within its bound of the float64 map; nothing in the image or the tile slots unwritten
  2 forward per tile      every tile's sums in the slot of THAT tile (the XCD remap on the device), the scalars
  3 backward in isolation the gradient against the float64 window sums of the maps the forward stored
  4 end to end            the gradient against float64 autograd of the published loss, tolerance = the composition of 1 and 3
  5 path equalities       bit for bit: offset by one float (the non-VEC kernels on a VEC-shaped image), _step, the shift design
A GPU run and its reference are made once per case and shared by the tests."""
import math

import numpy as np
import pytest
import torch

import photo_ref as R
from poison import fill_bytes

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
_RUNS = {}


def _dev(x, gpu, off):
    """x on the device, its first element `off` floats into a fresh allocation (off = 1: not 16-byte aligned)."""
    t = torch.from_numpy(np.ascontiguousarray(x, F32))
    buf = torch.empty(t.numel() + off, dtype=torch.float32, device=gpu)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


def launch(a, b, m, shape, lam, up, gpu, off=(0, 0, 0, 0), step=False):
    """forward + backward (or the _step entry) as _PhotoLoss does, on a poisoned workspace:
    (maps [3,C,H,W], tile sums [tiles, 2 | 3], parts [3 | 4], gradient [C,H,W]) as NumPy fp32."""
    from syn3r_amd import _lib as L
    from syn3r_amd.gs.train_ops import _photo_entries
    C, H, W = shape
    ta, tb = _dev(a, gpu, off[0]), _dev(b, gpu, off[1])
    tm = None if m is None else _dev(m, gpu, off[2])
    forward, backward, both, workspace_bytes, n_parts, name, map_ptr = _photo_entries(L.load(), tm)
    nbytes = workspace_bytes(C, H, W)
    buf = fill_bytes(torch.empty(nbytes + 4 * off[3], dtype=torch.uint8, device=gpu), 0xFF)
    ws = buf[4 * off[3]:]
    parts = fill_bytes(torch.empty(n_parts, dtype=torch.float32, device=gpu), 0xFF)
    grad = fill_bytes(torch.empty(shape, dtype=torch.float32, device=gpu), 0xFF)
    go = None if up is None else torch.tensor(up, dtype=torch.float32, device=gpu)
    st = L.stream_ptr(gpu)
    if step:
        L.check(both(L.ptr(ta), L.ptr(tb), *map_ptr, C, H, W, lam, R.WEIGHT, L.ptr(go), L.ptr(parts), L.ptr(grad), L.ptr(ws), nbytes, st),
                name + "_step")
    else:
        L.check(forward(L.ptr(ta), L.ptr(tb), *map_ptr, C, H, W, lam, R.WEIGHT, L.ptr(parts), L.ptr(ws), nbytes, st), name)
        L.check(backward(L.ptr(ta), L.ptr(tb), *map_ptr, C, H, W, lam, R.WEIGHT, L.ptr(go), L.ptr(ws), L.ptr(grad), st), name + "_backward")
    torch.cuda.synchronize()
    f = ws.cpu().numpy().view(F32)
    n, per = C * H * W, n_parts - 1
    tiles = C * R.grid(shape)[0] * R.grid(shape)[1]
    return (f[:3 * n].reshape(3, C, H, W).copy(), f[3 * n:3 * n + per * tiles].reshape(tiles, per).copy(), parts.cpu().numpy(),
            grad.cpu().numpy())


def run(case, gpu, off=(0, 0, 0, 0), step=False):
    key = (case.name, off, step)
    if key not in _RUNS:
        a, b, m, _ = case.data
        _RUNS[key] = launch(a, b, m, case.shape, case.lam, case.up, gpu, off, step)
    return _RUNS[key]


def is_equal(case):
    return case.family == "conditioning" and case.name.rsplit("-", 1)[0] in R.EQUAL


_CHECKED = {}


def check(case, k, gpu):
    """Check k on the case's cached run, evaluated once: the worst err / tol, or the CheckFailed it raised (returned, not raised)."""
    if (case.name, k) not in _CHECKED:
        maps, partial, parts, grad = run(case, gpu)
        ref = case.data[3]
        fn = {1: lambda: R.check_forward_pixels(ref, maps),
              2: lambda: R.check_forward_tiles(ref, partial, parts, case.lam, is_equal(case)),
              3: lambda: R.check_backward_isolated(ref, maps, grad, case.lam, case.up),
              4: lambda: R.check_end_to_end(ref, grad, case.lam, case.up)}[k]
        try:
            _CHECKED[(case.name, k)] = fn()
        except R.CheckFailed as e:
            _CHECKED[(case.name, k)] = e
    return _CHECKED[(case.name, k)]


def passes(case, k, gpu):
    w = check(case, k, gpu)
    if isinstance(w, R.CheckFailed):
        raise w
    print("err / tol %.4f" % w)


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_forward_per_pixel(case, gpu):
    maps, partial, _, _ = run(case, gpu)
    assert not np.isnan(maps).any() and not np.isnan(partial).any(), "the NaN pattern is left in the image or in a tile slot"
    passes(case, 1, gpu)


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_forward_per_tile(case, gpu):
    passes(case, 2, gpu)
    _, _, parts, _ = run(case, gpu)
    assert parts.shape == ((3,) if case.kind is None else (4,))


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_backward_in_isolation(case, gpu):
    passes(case, 3, gpu)
    if float(F32(case.lam)) == 1.0:            # the L1 term vanishes: c_l1 is exactly 0 and so is its share of the slack
        assert R.coefficients(case.shape, case.lam)[0] == 0


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_end_to_end(case, gpu):
    passes(case, 4, gpu)


WHAT = ("maps", "tile sums", "parts", "gradient")


@pytest.mark.parametrize("off", R.OFFSETS, ids=lambda o: "offset" + "".join(map(str, o)))
@pytest.mark.parametrize("case", [c for c in R.CASES if c.family == "alignment"], ids=repr)
def test_offset_by_one_float_equals_aligned(case, off, gpu):
    """A tensor (or the workspace) one float off a 16-byte boundary sends a VEC-shaped image through the non-VEC kernel: same bits."""
    for got, want, what in zip(run(case, gpu, off), run(case, gpu), WHAT):
        R.check_bits("%s at offsets %s" % (what, off), got, want)


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_step_equals_forward_then_backward(case, gpu):
    for got, want, what in zip(run(case, gpu, step=True), run(case, gpu), WHAT):
        R.check_bits("%s of the _step entry" % what, got, want)


def test_shift_design(gpu):
    """A 20 x 24 patch in a zero canvas, moved over tile borders and into the corners: over the patch and its surround the stored maps
    and the gradient keep their bits (zero padding and zero canvas are the same zeros, the taps of an output are accumulated in
    ascending order), for the VEC (W = 84) and the non-VEC (W = 83) kernels; the far field holds -rcp(C2) in d_sg1."""
    runs = {}
    for canvas in R.CANVASES:
        for offset in [R.CANONICAL] + R.SHIFTS:
            a, b = R.shift_images(canvas, offset)
            maps, _, _, grad = launch(a, b, None, canvas, 0.2, 1.5, gpu)
            runs[(canvas, offset)] = (maps, grad)
    R.check_shift(runs)


def _published_fp32(a, b):
    """The published formula evaluated in fp32 by torch on the CPU: the SSIM map."""
    import torch.nn.functional as Fn
    a, b = torch.from_numpy(a), torch.from_numpy(b)
    g = torch.tensor([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum())[:, None]
    C = a.shape[0]
    win = (g @ g.t())[None, None].expand(C, 1, 11, 11).contiguous()
    conv = lambda t: Fn.conv2d(t[None], win, padding=5, groups=C)[0]
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).numpy()


def _tile_means(v, shape):
    C, H, W = shape
    gy, gx = R.grid(shape)
    p = np.zeros((C, gy * R.TILE, gx * R.TILE))
    p[:, :H, :W] = v
    return p.reshape(C, gy, R.TILE, gx, R.TILE).sum(axis=(2, 4)).reshape(-1)


def test_recorded_figures(gpu, measurements):
    """Recorded, not asserted: per family the worst err / tol of checks 1 to 4; on the conditioning designs the error of parts[2] and
    of the worst tile mean against float64, beside the same figures of the published formula in fp32 on the CPU; max|grad| at
    image == target relative to c_l1."""
    worst = {}
    for case in R.CASES:
        for k in (1, 2, 3, 4):
            w = check(case, k, gpu)
            w = w.worst if isinstance(w, R.CheckFailed) else w
            worst[(case.family, k)] = max(worst.get((case.family, k), 0.0), w)
    for (family, k), w in sorted(worst.items()):
        print("%-12s check %d: worst err / tol %.4f" % (family, k, w))
        measurements("photo_elementwise_worst", family=family, check=k, err_over_tol=w)
    for case in R.CASES:
        if case.family != "conditioning":
            continue
        a, b, _, ref = case.data
        _, partial, parts, grad = run(case, gpu)
        pref, _ = ref.parts(case.lam)
        mean_ref = ref.tile_sums[:, 1] / ref.count
        cpu = _published_fp32(a, b).astype(F64)
        fig = dict(kernel_parts2_err=abs(float(parts[2]) - pref[2]), cpu_fp32_parts2_err=abs(float(cpu.mean()) - pref[2]),
                   kernel_tile_mean_err=float(np.abs(partial[:, 1].astype(F64) / ref.count - mean_ref).max()),
                   cpu_fp32_tile_mean_err=float(np.abs(_tile_means(cpu, case.shape) / ref.count - mean_ref).max()))
        if is_equal(case):
            fig["grad_max_over_c_l1"] = float(np.abs(grad).max() / float(R.coefficients(case.shape, case.lam)[0]))
        print(case.name, " ".join("%s %.3g" % kv for kv in fig.items()))
        measurements("photo_elementwise_conditioning", case=case.name, **fig)
