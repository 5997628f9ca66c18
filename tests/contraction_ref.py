"""Exact-sum designs and the bit-exact model of the contraction kernels (csrc/gemm.hip and its gemm_*.h families).

Host only (numpy + torch; `device` is where the float64 matmul runs, "cpu" by default).

Operands: A on the 1/8 grid in [-2, 2], W on the 1/16 grid in [-1, 1].  Every product is a multiple of 2^-7 and every partial
sum over K <= 11 520 stays far below 2^24 units of that grid, so the fp32 accumulator of ANY summation order (k-tiles, split-K,
tap order, lane-split + wave sum) holds the exact sum, and float64 holds the same value.  Bias, row vector, residual and aux are
on the 1/8 grid, the scales have at most three mantissa bits, so every fp32 operation of the epilogue is exact too and the only
roundings are the two fp16 conversions the kernels make:

    stage = f16((acc + bias + rowvec) * s_acc)
    out   = f16(stage + s_res * residual + s_aux * aux)

A case is (kind, shape, variant):
    kind     "dense" (M, N, K) | "conv_s1" / "conv_s2p1" / "conv_s2p0" / "conv_ups" (NB, Hi, Wi, Cin, Cout)
             | "tconv" (B, F, HW, Cin, Cout) | "two_src" (M, N, K1, K2) | "gated" (M, D, K) (the projection [hidden | gate], N = 2 D)
    variant  a key of EPILOGUES
"""
import zlib

import numpy as np
import torch

F64 = torch.float64
H = torch.float16
SENTINEL_BITS = 0x7E00          # an fp16 NaN: never equal to an expected value, poisons every sum it enters
EXTRA_ROWS = 16

# rowvec = (rows_per_vec, rv_group_rows); "image": one vector per image (conv: Ho * Wo rows) / per clip (tconv: F * HW rows)
EPILOGUES = {
    "none": dict(bias=False),
    "bias": dict(s_acc=0.5),
    "bias1": dict(),                               # the entries without scales (two-source, gated, four-phase upsample)
    "rv100": dict(rowvec=(100, 0), s_acc=0.75),
    "rv-8": dict(rowvec=(-8, 0), s_acc=1.25),
    "rv-4g52": dict(rowvec=(-4, 52), s_acc=0.5),
    "res": dict(residual=True, s_acc=0.75, s_res=0.625),
    "res_aux": dict(residual=True, aux=True, s_acc=1.25, s_res=1.0, s_aux=0.375),
    "aux": dict(aux=True, s_acc=1.0, s_aux=0.375),
    "rv_img_res": dict(rowvec=("image", 0), residual=True, s_acc=0.75, s_res=0.625),
    "full": dict(rowvec=(100, 0), residual=True, aux=True, s_acc=0.75, s_res=0.625, s_aux=0.375),
}

CONV_GEOM = {"conv_s1": (1, 1, False), "conv_s2p1": (2, 1, False), "conv_s2p0": (2, 0, False), "conv_ups": (1, 1, True)}   # stride, pad_lo, upsample

# ---- shape lists -----------------------------------------------------------------------------------------------------------
TILES = (0, -128, -256, -320, -322)
_M, _N, _K = (8, 37, 129, 264, 520), (8, 48, 160, 168, 320, 328, 648), (64, 128, 192, 320, 640)
DENSE_EPILOGUES = ("none", "bias", "rv100", "rv-8", "rv-4g52", "res", "res_aux", "aux")
# every (M, N) pair; K walks its five values along both axes (every M and every N meets every k-tile count); N = 150: scalar tail stores
DENSE_SHAPES = [(m, n, _K[(i + j) % 5]) for i, m in enumerate(_M) for j, n in enumerate(_N)] + [(37, 150, 64), (264, 150, 192)]
DENSE_SMALL = [("dense", s, v) for s in DENSE_SHAPES for v in DENSE_EPILOGUES]
MANY_EPILOGUES = ("none", "res", "res_aux", "rv100", "rv-8")
DENSE_WIDE_MANY = [("dense", (2056, 9608, k), v) for k in (128, 192) for v in MANY_EPILOGUES]         # 9 x 31 tiles of 256 x 320
DENSE_DMAP_MANY = [("dense", (2056, 4808, 192), v) for v in MANY_EPILOGUES]                            # 9 x 31 tiles of 256 x 160
DENSE_DMAPD = [("dense", (8448, 1280, 640), "res"), ("dense", (8448, 1280, 1280), "bias"),              # 264 whole tiles
               ("dense", (8448, 1280, 1280), "rv100"), ("dense", (8448, 1280, 1280), "rv-8")]
DENSE = DENSE_SMALL + DENSE_WIDE_MANY + DENSE_DMAP_MANY + DENSE_DMAPD

CONV_SHAPES = [(2, 5, 7, 64, 160), (3, 9, 16, 128, 328), (2, 10, 12, 192, 64)]
CONV_SMALL = [(k, s, v) for s in CONV_SHAPES for k, v in (("conv_s1", "bias"), ("conv_s2p1", "bias"), ("conv_s2p0", "bias"),
                                                          ("conv_ups", "bias"), ("conv_s1", "rv_img_res"))]
CONV_MANY = [("conv_s1", (2, 33, 32, 64, 9608), "bias"), ("conv_ups", (2, 17, 16, 64, 9608), "bias")]   # M = 2112: 9 x 31 tiles
UP4 = [("conv_ups", s, "bias1") for s in CONV_SHAPES + [CONV_MANY[1][1]]]                                    # 4 x 3 x 31 = 372 tiles
CONV = CONV_SMALL + CONV_MANY

# (M = 80: the only one with M % 8 == 0, which k_gemm_z<2> asks for)
TCONV_SMALL = [("tconv", s, "res") for s in ((2, 5, 7, 64, 160), (1, 25, 30, 128, 320), (2, 3, 13, 64, 336), (2, 5, 8, 64, 328))]
TCONV_MANY = [("tconv", (2, 6, 256, 64, 4808), "res")]              # frame-minor tile order, 12 x 31 = 372 tiles
TCONV = TCONV_SMALL + TCONV_MANY

TWO_SRC_SMALL = [("two_src", (m, n, k1, k2), "bias1") for (m, n) in ((264, 328), (520, 168)) for (k1, k2) in ((64, 64), (128, 64), (64, 192))]
TWO_SRC_MANY = [("two_src", (2056, 9608, 64, 128), "bias1")]
TWO_SRC = TWO_SRC_SMALL + TWO_SRC_MANY

SKINNY = [("dense", (m, n, k), v) for m in (1, 2, 3, 8, 9, 16) for n in (8, 161, 162, 1280) for k in (64, 512, 1280) for v in ("none", "bias")]

# (case, number of K parts the dispatch gives it)
SPLITK = [(("dense", (264, 320, 512), "full"), 2), (("dense", (264, 320, 1024), "full"), 4), (("conv_s1", (4, 8, 8, 128, 160), "rv_img_res"), 2),
          (("tconv", (2, 6, 20, 256, 192), "rv_img_res"), 2), (("two_src", (264, 320, 256, 256), "bias1"), 2)]

GEGLU_SMALL = [("gated", (m, d, k), "bias1") for m in (37, 520) for d in (80, 200, 640) for k in (64, 192, 320)]
GEGLU_MANY = [("gated", (2056, 4800, 128), "bias1")]                 # 9 x 30 tiles
FF_PLAIN = [("gated", s, "bias1") for s in ((37, 128, 64), (520, 640, 192), (37, 640, 192), (520, 128, 64))]
FF_P64 = [("gated", (m, 128, k), "bias1") for m in (256, 384) for k in (128, 320)] + [("gated", (2432, 3584, 128), "bias1")]   # 10 x 28 tiles of 256 x 256
FF_FUSED = [("gated", (m, d, 320), "bias1") for m in (129, 700) for d in (64, 1280)]
GATED = GEGLU_SMALL + GEGLU_MANY + FF_PLAIN + FF_P64 + FF_FUSED

ALL_CASES = list(dict.fromkeys(DENSE + CONV + UP4 + TCONV + TWO_SRC + SKINNY + [c for c, _ in SPLITK] + GATED))

# a case whose first seed does not meet a condition of the design gets another one here (tests/test_contraction_exact_cpu.py
# says which condition: unit coverage, or a residual case whose reference never rounds twice)
SEED_BUMP = {("dense", (8, 8, 64), "res_aux"): 1,                 # 64 elements, none rounded twice with the first seed
             ("dense", (129, 648, 320), "none"): 2, ("dense", (129, 648, 320), "rv100"): 1, ("dense", (129, 648, 320), "aux"): 1,
             ("dense", (1, 1280, 64), "none"): 1}               # an exact zero in a one-row unit (row 128 / the only row)


def case_id(case) -> str:
    kind, shape, variant = case
    return f"{kind}-{'x'.join(map(str, shape))}-{variant}"


def dims(case):
    """(M, N, K) of the contraction a case amounts to."""
    kind, s, _ = case
    if kind == "dense":
        return s
    if kind in CONV_GEOM:
        stride, pad_lo, ups = CONV_GEOM[kind]
        NB, Hi, Wi, Cin, Cout = s
        Hg, Wg = (2 * Hi, 2 * Wi) if ups else (Hi, Wi)
        return NB * ((Hg + pad_lo - 2) // stride + 1) * ((Wg + pad_lo - 2) // stride + 1), Cout, 9 * Cin
    if kind == "tconv":
        return s[0] * s[1] * s[2], s[4], 3 * s[3]
    if kind == "two_src":
        return s[0], s[1], s[2] + s[3]
    if kind == "gated":
        return s[0], 2 * s[1], s[2]
    raise ValueError(kind)


def rowvec_rows(M: int, rows_per_vec: int, rv_group_rows: int = 0) -> np.ndarray:
    """Which row of the vector table row m adds: the three forms of include/syn3r_hip.h (syn3r_gemm_f16)."""
    m = np.arange(M)
    if rows_per_vec > 0:
        return m // rows_per_vec
    P = -rows_per_vec
    return (m // rv_group_rows * P if rv_group_rows > 0 else 0) + m % P


def _grid(rng, shape, denom, lim):
    return rng.randint(-lim * denom, lim * denom + 1, size=shape).astype(np.float64) / denom


def design(case, seed=None) -> dict:
    """The dyadic operands of a case as float64 numpy arrays (independent draws: the values vary along every axis), with the
    epilogue terms of its variant.  Keys: the operands of the kind (A, W | X, W | A1, A2, W), bias [N], rowvec [V, N] with
    rows_per_vec / rv_group_rows, residual / aux [M, N], s_acc / s_res / s_aux; absent terms are None."""
    kind, s, variant = case
    if seed is None:
        seed = (zlib.crc32(case_id(case).encode()) + SEED_BUMP.get(case, 0)) & 0x7FFFFFFF
    rng = np.random.RandomState(seed)
    M, N, K = dims(case)
    d = dict(case=case, kind=kind, shape=s, M=M, N=N, K=K)
    if kind in ("dense", "gated"):
        d["A"] = _grid(rng, (M, K), 8, 2)
        d["W"] = _grid(rng, (N, K), 16, 1)
    elif kind in CONV_GEOM:
        NB, Hi, Wi, Cin, Cout = s
        d["X"] = _grid(rng, (NB, Hi, Wi, Cin), 8, 2)                  # NHWC
        d["W"] = _grid(rng, (Cout, 3, 3, Cin), 16, 1)                 # OHWI
    elif kind == "tconv":
        B, F, HW, Cin, Cout = s
        d["X"] = _grid(rng, (M, Cin), 8, 2)
        d["W"] = _grid(rng, (Cout, 3, Cin), 16, 1)
    elif kind == "two_src":
        d["A1"], d["A2"] = _grid(rng, (M, s[2]), 8, 2), _grid(rng, (M, s[3]), 8, 2)
        d["W"] = _grid(rng, (N, K), 16, 1)
    e = dict(bias=True, rowvec=None, residual=False, aux=False, s_acc=1.0, s_res=1.0, s_aux=1.0)
    e.update(EPILOGUES[variant])
    d["bias"] = _grid(rng, (N,), 8, 2) if e["bias"] else None
    d["rowvec"], d["rows_per_vec"], d["rv_group_rows"] = None, 0, 0
    if e["rowvec"] is not None:
        rpv, G = e["rowvec"]
        if rpv == "image":
            rpv = s[1] * s[2] if kind == "tconv" else M // s[0]
        d["rows_per_vec"], d["rv_group_rows"] = rpv, G
        d["rowvec"] = _grid(rng, (int(rowvec_rows(M, rpv, G).max()) + 1, N), 8, 2)
    d["residual"] = _grid(rng, (M, N), 8, 2) if e["residual"] else None
    d["aux"] = _grid(rng, (M, N), 8, 2) if e["aux"] else None
    d["s_acc"], d["s_res"], d["s_aux"] = e["s_acc"], e["s_res"], e["s_aux"]
    return d


def _t(a, device):
    return None if a is None else torch.as_tensor(a, dtype=F64).to(device)


def im2col3x3(x, stride=1, pad_lo=1, upsample=False, *, clamp=False, yshift=0, ups_bias=0):
    """x [NB, Hi, Wi, C] -> [NB * Ho * Wo, 9 C], columns (ty, tx, c): the A matrix of the 3x3 convolution on the (nearest-2x
    upsampled) image with pad_lo zero rows / columns before it and zeros wherever the window runs past it.
    clamp / yshift / ups_bias restate WRONG gathers (the mutants of the CPU test): the edge pixel instead of the zero, window rows
    moved down by yshift, the upsample reading (g + ups_bias) // 2."""
    x = torch.as_tensor(x)
    NB, Hi, Wi, C = x.shape
    Hg, Wg = (2 * Hi, 2 * Wi) if upsample else (Hi, Wi)
    Ho, Wo = (Hg + pad_lo - 2) // stride + 1, (Wg + pad_lo - 2) // stride + 1
    xp = torch.zeros((NB, Hi + 1, Wi + 1, C), dtype=x.dtype, device=x.device)       # row Hi / column Wi: the zero pixel
    xp[:, :Hi, :Wi] = x

    def src(n_out, n_g, n_in, tap, shift):
        g = torch.arange(n_out, device=x.device) * stride + tap - pad_lo + shift
        inside = (g >= 0) & (g < n_g)
        if clamp:
            g, inside = g.clamp(0, n_g - 1), torch.ones_like(inside)
        i = ((g + ups_bias) // 2).clamp(0, n_in - 1) if upsample else g
        return torch.where(inside, i, torch.full_like(i, n_in))
    taps = [xp[:, src(Ho, Hg, Hi, ty, yshift)[:, None], src(Wo, Wg, Wi, tx, 0)[None, :], :] for ty in range(3) for tx in range(3)]
    return torch.cat(taps, dim=-1).reshape(NB * Ho * Wo, 9 * C)


def tconv_rows(x, B, F, HW, *, wrap_clips=False):
    """x [B F HW, C] -> [B F HW, 3 C], columns (tap, c): frames f - 1, f, f + 1 of the same pixel, zero frames at both ends of every
    clip.  wrap_clips restates a WRONG gather: frame f - 1 of a clip's first frame is the previous clip's last one."""
    x = torch.as_tensor(x)
    C = x.shape[1]
    x4 = x.reshape(B, F, HW, C)
    z = torch.zeros_like(x4[:, :1])
    prev, nxt = torch.cat([z, x4[:, :-1]], 1), torch.cat([x4[:, 1:], z], 1)
    if wrap_clips:
        prev = torch.cat([torch.zeros_like(x[:HW]), x[:-HW]], 0).reshape(B, F, HW, C)
    return torch.cat([prev, x4, nxt], dim=-1).reshape(B * F * HW, 3 * C)


def operands(d, device="cpu"):
    """(A [M, K], W [N, K]) float64: the matrices whose product the case's kernel accumulates (explicit im2col for the convolutions)."""
    kind = d["kind"]
    W = _t(d["W"], device).reshape(d["N"], d["K"])
    if kind in ("dense", "gated"):
        return _t(d["A"], device), W
    if kind in CONV_GEOM:
        stride, pad_lo, ups = CONV_GEOM[kind]
        return im2col3x3(_t(d["X"], device), stride, pad_lo, ups), W
    if kind == "tconv":
        B, F, HW = d["shape"][:3]
        return tconv_rows(_t(d["X"], device), B, F, HW), W
    return torch.cat([_t(d["A1"], device), _t(d["A2"], device)], 1), W


def f16(x):
    """float64 -> fp16, one rounding to nearest even (through fp32: every value this module rounds is an fp32 number)."""
    return torch.as_tensor(x).to(torch.float32).to(H)


def two_cast(acc, bias=None, rv=None, residual=None, aux=None, s_acc=1.0, s_res=1.0, s_aux=1.0):
    """The epilogue of every contraction kernel on an exactly known accumulator (float64 tensors or arrays) -> fp16 tensor."""
    acc = torch.as_tensor(acc, dtype=F64)
    dev = acc.device
    v = acc
    if bias is not None:
        v = v + torch.as_tensor(bias, dtype=F64).to(dev)
    if rv is not None:
        v = v + torch.as_tensor(rv, dtype=F64).to(dev)
    out = f16(v * s_acc)
    if residual is None and aux is None:
        return out
    v = out.to(F64)
    if residual is not None:
        v = v + s_res * torch.as_tensor(residual, dtype=F64).to(dev)
    if aux is not None:
        v = v + s_aux * torch.as_tensor(aux, dtype=F64).to(dev)
    return f16(v)


def _sel(t, rows, cols):
    if t is None:
        return None
    if rows is not None:
        t = t[rows]
    if cols is not None:
        t = t[:, cols]
    return t


def terms(d, device="cpu", rows=None, cols=None):
    """The epilogue terms of (a row / column selection of) the output: bias [n], the gathered row vectors [m, n], residual, aux."""
    rows = None if rows is None else torch.as_tensor(rows, device=device)
    cols = None if cols is None else torch.as_tensor(cols, device=device)
    bias = _t(d["bias"], device)
    if bias is not None and cols is not None:
        bias = bias[cols]
    rv = None
    if d["rowvec"] is not None:
        idx = torch.as_tensor(rowvec_rows(d["M"], d["rows_per_vec"], d["rv_group_rows"]), device=device)
        rv = _sel(_t(d["rowvec"], device)[idx if rows is None else idx[rows]], None, cols)
    return bias, rv, _sel(_t(d["residual"], device), rows, cols), _sel(_t(d["aux"], device), rows, cols)


def accumulate(d, device="cpu", rows=None, cols=None):
    A, W = operands(d, device)
    if rows is not None:
        A = A[torch.as_tensor(rows, device=device)]
    if cols is not None:
        W = W[torch.as_tensor(cols, device=device)]
    return A @ W.T


def expected(d, device="cpu", rows=None, cols=None):
    """The fp16 output of the case, bit for bit ([M, N], or the selected rows / columns of it), on `device`."""
    bias, rv, res, aux = terms(d, device, rows, cols)
    return two_cast(accumulate(d, device, rows, cols), bias, rv, res, aux, d["s_acc"], d["s_res"], d["s_aux"])


def sample_rows_cols(M, N, max_rows=96, max_cols=64):
    """Whole 16-row / 8-column units from the start, the middle and the (ragged) end of a large output; (None, None) = all of it."""
    def pick(n, unit, limit):
        if n <= limit:
            return None
        last, mid = (n - 1) // unit * unit, (n // 2) // unit * unit
        k = limit // unit // 3 * unit
        return np.unique(np.concatenate([np.arange(k), np.arange(mid, mid + k), np.arange(max(last - k + unit, 0), n)]))
    return pick(M, 16, max_rows), pick(N, 8, max_cols)


def check_exactness(d, device="cpu", rows=None, cols=None):
    """The conditions on the INPUTS the bit-exact model rests on; returns the expected output of the selection."""
    A, W = operands(d, device)
    r = torch.arange(d["M"], device=device) if rows is None else torch.as_tensor(rows, device=device)
    c = torch.arange(d["N"], device=device) if cols is None else torch.as_tensor(cols, device=device)
    A, W = A[r], W[c]
    # 1. every partial sum, in any order, is an integer below 2^24 on the 2^-7 grid
    assert ((A * 8) == (A * 8).round()).all() and ((W * 16) == (W * 16).round()).all(), case_id(d["case"])
    bound = (A.abs() @ W.abs().T).max().item() * 128
    assert bound < 2 ** 24, (case_id(d["case"]), bound)
    # 2. staged and final values are finite fp16 numbers, and the epilogue's fp32 operations are exact (24 bits on their grids)
    bias, rv, res, aux = terms(d, device, rows, cols)
    acc = A @ W.T
    pre = acc + (0 if bias is None else bias) + (0 if rv is None else rv)
    assert (pre.abs() * 128).max().item() < 2 ** 24
    stage = f16(pre * d["s_acc"]).to(F64)
    assert ((pre * d["s_acc"]).abs() < 65504).all() and torch.isfinite(stage).all()
    fin = stage + (0 if res is None else d["s_res"] * res) + (0 if aux is None else d["s_aux"] * aux)
    assert (fin * 512 == (fin * 512).round()).all() and (fin.abs() * 512).max().item() < 2 ** 24
    assert (fin.abs() < 65504).all()
    out = f16(fin)
    assert torch.isfinite(out).all()
    # 3. non-zero on >= 90 % of every 16-row x 8-column unit of the output (a missing store shows, a dropped product changes a value)
    ur, uc = torch.unique(r // 16, return_inverse=True)[1], torch.unique(c // 8, return_inverse=True)[1]
    R = torch.zeros((int(ur.max()) + 1, len(r)), dtype=F64, device=device)
    R[ur, torch.arange(len(r), device=device)] = 1
    C = torch.zeros((len(c), int(uc.max()) + 1), dtype=F64, device=device)
    C[torch.arange(len(c), device=device), uc] = 1
    nz, size = R @ (out != 0).to(F64) @ C, R @ torch.ones_like(acc) @ C
    assert (nz >= 0.9 * size).all(), (case_id(d["case"]), "a unit of the expected output is zero on more than 10 % of its elements")
    return out


# ---- sentinel-framed buffers -----------------------------------------------------------------------------------------------
def ldc_of(N: int) -> int:
    return (N + 7) // 8 * 8 + 8


def sentinel(shape, device="cpu"):
    return torch.full(shape, SENTINEL_BITS, dtype=torch.int16, device=device).view(H)


def framed(exp, ldc=None):
    """`exp` [M, N] inside a sentinel-filled [M + 16, ldc] buffer: what an `out=` buffer must hold after the call."""
    M, N = exp.shape
    buf = sentinel((M + EXTRA_ROWS, ldc or ldc_of(N)), exp.device)
    buf[:M, :N] = exp
    return buf


def compare(got_buf, want_buf, M, N):
    """(number of differing elements inside [M, N], the sentinel outside is intact, a printable report of the differences)."""
    got, want = got_buf[:M, :N], want_buf[:M, :N]
    bad = ~(got == want)                                   # a NaN that was never overwritten differs too
    frame = got_buf.view(torch.int16).clone()
    frame[:M, :N] = SENTINEL_BITS
    intact = bool((frame == SENTINEL_BITS).all())
    n = int(bad.sum())
    report = ""
    if n or not intact:
        idx = bad.nonzero()[:6].cpu()
        first = [(int(m), int(c), float(got[m, c]), float(want[m, c])) for m, c in idx]
        tiles = sorted({(int(m) // 128, int(c) // 160) for m, c in bad.nonzero()[:: max(1, n // 4096)].cpu()})
        stray = (frame != SENTINEL_BITS).nonzero()[:6].cpu().tolist()
        report = f"{n} of {M * N} differ; first (m, n, got, want): {first}; (m // 128, n // 160) tiles: {tiles[:40]}; writes outside [M, N]: {stray}"
    return n, intact, report
