"""The exact-sum designs of tests/contraction_ref.py, without a GPU.

  * every design of the shape lists meets `check_exactness` (a row / column sample of whole 16 x 8 units for the large ones);
  * an fp32 restatement of the contraction equals the float64 reference exactly in four orders (ascending k, descending k, four K
    parts summed pairwise, the BLAS's own): the bit-exact model does not depend on the order a kernel sums in;
  * numpy restatements of subtly wrong kernels (one k-tile dropped, a swizzle undone, a clamped border, a single rounding ...) all
    differ from `expected`, in the place the flaw sits where that is known.
"""
import numpy as np
import pytest
import torch

import contraction_ref as R

F64, F32, F16 = np.float64, np.float32, np.float16


def _np(t):
    return t.detach().cpu().numpy()


def _sample(case):
    M, N, _ = R.dims(case)
    return R.sample_rows_cols(M, N) if M * N > 1 << 18 else (None, None)


@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_design_is_exact_in_every_order(case):
    d = R.design(case)
    rows, cols = _sample(case)
    R.check_exactness(d, rows=rows, cols=cols)
    A, W = R.operands(d)
    A, W = _np(A if rows is None else A[rows])[:48], _np(W if cols is None else W[cols])[:48]
    ref = A @ W.T                                             # float64
    a32, w32 = A.astype(F32), W.astype(F32)
    assert np.array_equal(a32.astype(F64), A) and np.array_equal(w32.astype(F64), W)
    K = A.shape[1]
    up, down = np.zeros(ref.shape, F32), np.zeros(ref.shape, F32)
    for k in range(K):
        up += a32[:, k, None] * w32[None, :, k]
        down += a32[:, K - 1 - k, None] * w32[None, :, K - 1 - k]
    q = K // 4
    parts = [np.zeros(ref.shape, F32) for _ in range(4)]
    for i in range(4):
        for k in range(i * q, (i + 1) * q if i < 3 else K):
            parts[i] += a32[:, k, None] * w32[None, :, k]
    pairwise = (parts[0] + parts[1]) + (parts[2] + parts[3])
    for name, got in (("ascending", up), ("descending", down), ("pairwise", pairwise), ("blas", a32 @ w32.T)):
        assert got.dtype == F32 and np.array_equal(got.astype(F64), ref), (R.case_id(case), name)


def test_rowvec_rows_forms():
    assert R.rowvec_rows(7, 3).tolist() == [0, 0, 0, 1, 1, 1, 2]
    assert R.rowvec_rows(7, -3).tolist() == [0, 1, 2, 0, 1, 2, 0]
    assert R.rowvec_rows(9, -2, 4).tolist() == [0, 1, 0, 1, 2, 3, 2, 3, 4]          # group g of 4 rows reads vectors 2 g + m mod 2


def test_im2col_against_direct_sum():
    """The explicit im2col of the reference against a per-pixel loop written from the definition (all four geometries)."""
    rng = np.random.RandomState(3)
    x = rng.randint(-16, 17, size=(2, 5, 6, 3)).astype(F64)
    for kind, (stride, pad_lo, ups) in R.CONV_GEOM.items():
        g = np.repeat(np.repeat(x, 2, 1), 2, 2) if ups else x
        Hg, Wg = g.shape[1:3]
        gp = np.zeros((2, Hg + 3, Wg + 3, 3))
        gp[:, pad_lo:pad_lo + Hg, pad_lo:pad_lo + Wg] = g
        Ho, Wo = (Hg + pad_lo - 2) // stride + 1, (Wg + pad_lo - 2) // stride + 1
        want = np.stack([gp[n, y * stride:y * stride + 3, xx * stride:xx * stride + 3].reshape(-1)
                         for n in range(2) for y in range(Ho) for xx in range(Wo)])
        assert np.array_equal(_np(R.im2col3x3(x, stride, pad_lo, ups)), want), kind


# ---------------------------------------------------------------------------------------------------------------- mutants
def _model(d, A=None, W=None, acc=None, bias=None, rv=None, **kw):
    """`expected` with parts of it replaced (numpy in, numpy fp16 out)."""
    A0, W0 = R.operands(d)
    b0, rv0, res, aux = R.terms(d)
    if acc is None:
        acc = (_np(A0) if A is None else A) @ (_np(W0) if W is None else W).T
    s = dict(s_acc=d["s_acc"], s_res=d["s_res"], s_aux=d["s_aux"])
    return _np(R.two_cast(acc, b0 if bias is None else bias, rv0 if rv is None else rv, res, aux, **s))


def _differs(got, want, where=None):
    """The mutant's output differs from the expected one - inside `where` (a boolean mask) and nowhere else, when given."""
    bad = got.view(np.uint16) != want.view(np.uint16)
    assert bad.any()
    if where is not None:
        assert not (bad & ~where).any() and bad[where].mean() > 0.5, bad[where].mean()


FULL = ("dense", (264, 328, 320), "full")          # bias, rows_per_vec = 100, residual, aux, three scales


def _mask(shape, rows, cols):
    m = np.zeros(shape, bool)
    m[rows, cols] = True
    return m


def test_mutant_k_tile_skipped_or_doubled():
    d = R.design(FULL)
    want = _np(R.expected(d))
    A, W = map(_np, R.operands(d))
    acc = A @ W.T
    part = A[:256, 64:128] @ W[160:320, 64:128].T               # k-tile 1 of row tile 0, column band 1
    where = _mask(acc.shape, slice(0, 256), slice(160, 320))
    for sign in (-1, +1):
        m = acc.copy()
        m[:256, 160:320] += sign * part
        _differs(_model(d, acc=m), want, where)


@pytest.mark.parametrize("case", [c for c in R.DENSE_SMALL + R.GEGLU_SMALL + R.CONV_SMALL + R.TCONV_SMALL if R.dims(c)[2] >= 320 and c[2] in ("bias", "bias1", "res", "rv_img_res")],
                         ids=R.case_id)
def test_mutant_fp16_accumulation(case):
    d = R.design(case)
    A, W = map(_np, R.operands(d))
    A, W = A[:64], W[:64]
    acc = np.zeros((A.shape[0], W.shape[0]), F16)
    for k in range(A.shape[1]):
        acc = (acc.astype(F32) + A[:, k, None].astype(F32) * W[None, :, k].astype(F32)).astype(F16)
    exact = A @ W.T
    assert (acc.astype(F64) != exact).mean() > 0.1              # (29 % at K = 320 in the issue's measurement; rounded once: less)
    r, c = np.arange(A.shape[0]), np.arange(W.shape[0])
    b, rv, res, aux = R.terms(d, rows=r, cols=c)
    s = dict(s_acc=d["s_acc"], s_res=d["s_res"], s_aux=d["s_aux"])
    _differs(_np(R.two_cast(acc.astype(F64), b, rv, res, aux, **s)), _np(R.two_cast(exact, b, rv, res, aux, **s)))


def test_mutant_a_rows_swapped_in_a_group():
    d = R.design(FULL)
    A, _ = map(_np, R.operands(d))
    m = A.copy()
    m[16:32] = A[np.arange(16, 32) ^ 1]
    _differs(_model(d, A=m), _np(R.expected(d)), _mask((d["M"], d["N"]), slice(16, 32), slice(None)))


def test_mutant_w_swizzle_undone_for_one_chunk():
    """LDS rows hold their 16-byte chunks XOR-swizzled (chunk ^ (row & 7)); a fragment read of chunk 3 of k-tile 0 without the
    swizzle gets logical chunk 3 ^ (n & 7)."""
    d = R.design(FULL)
    _, W = map(_np, R.operands(d))
    m = W.copy()
    for n in range(160):
        c = 3 ^ (n & 7)
        m[n, 24:32] = W[n, 8 * c:8 * c + 8]
    where = _mask((d["M"], d["N"]), slice(None), [n for n in range(160) if n & 7])
    _differs(_model(d, W=m), _np(R.expected(d)), where)


CONV_A = ("conv_s1", (3, 9, 16, 128, 328), "bias")


def _conv_mutant(case, **flaw):
    d = R.design(case)
    stride, pad_lo, ups = R.CONV_GEOM[case[0]]
    good, bad = _np(R.im2col3x3(d["X"], stride, pad_lo, ups)), _np(R.im2col3x3(d["X"], stride, pad_lo, ups, **flaw))
    touched = (good != bad).any(1)
    assert touched.any()
    _differs(_model(d, A=bad), _np(R.expected(d)), np.broadcast_to(touched[:, None], (d["M"], d["N"])))
    return d, touched


def test_mutant_conv_padding_clamped():
    d, touched = _conv_mutant(CONV_A, clamp=True)
    NB, Hi, Wi = d["shape"][:3]
    y, x = np.divmod(np.arange(d["M"]) % (Hi * Wi), Wi)
    assert np.array_equal(touched, (y == 0) | (y == Hi - 1) | (x == 0) | (x == Wi - 1))      # the border pixels, all of them
    _conv_mutant(("conv_s2p0", (2, 10, 12, 192, 64), "bias"), clamp=True)
    _conv_mutant(("conv_ups", (2, 5, 7, 64, 160), "bias"), clamp=True)


@pytest.mark.parametrize("kind", ["conv_s2p1", "conv_s2p0"])
def test_mutant_conv_stride2_row_off_by_one(kind):
    _, touched = _conv_mutant((kind, (3, 9, 16, 128, 328), "bias"), yshift=1)
    assert touched.all()


def test_mutant_conv_upsample_rounds_up():
    _, touched = _conv_mutant(("conv_ups", (3, 9, 16, 128, 328), "bias"), ups_bias=1)
    assert touched.mean() > 0.9            # (the last row / column of an image clamp to the same source pixel either way)


def test_mutant_tconv_previous_clip():
    case = ("tconv", (2, 5, 7, 64, 160), "res")
    d = R.design(case)
    B, F, HW = case[1][:3]
    bad = _np(R.tconv_rows(d["X"], B, F, HW, wrap_clips=True))
    where = _mask((d["M"], d["N"]), slice(F * HW, F * HW + HW), slice(None))        # frame 0 of clip 1
    _differs(_model(d, A=bad), _np(R.expected(d)), where)


def test_mutant_two_source_first_tile_of_a2():
    case = ("two_src", (264, 328, 128, 64), "bias1")
    d = R.design(case)
    A, _ = map(_np, R.operands(d))
    m = A.copy()
    m[:, 128:192] = A[:, 0:64]
    _differs(_model(d, A=m), _np(R.expected(d)), np.ones((264, 328), bool))


def test_mutant_rowvec_index():
    d = R.design(("dense", (264, 328, 320), "rv100"))
    want = _np(R.expected(d))
    idx = R.rowvec_rows(264, 100)
    last = np.arange(264) % 100 == 99
    bad = np.minimum(idx + last, len(d["rowvec"]) - 1)
    _differs(_model(d, rv=d["rowvec"][bad]), want, _mask(want.shape, [99, 199], slice(None)))
    g = R.design(("dense", (264, 328, 320), "rv-4g52"))
    flat = R.rowvec_rows(264, -4, 0)
    _differs(_model(g, rv=g["rowvec"][flat]), _np(R.expected(g)), _mask(want.shape, slice(52, 264), slice(None)))


def test_mutant_residual_before_scale():
    d = R.design(FULL)
    acc = _np(R.accumulate(d))
    b, rv, res, aux = map(_np, R.terms(d))
    m = R.two_cast(acc + res, b, rv, None, aux, d["s_acc"], 1.0, d["s_aux"])
    _differs(_np(m), _np(R.expected(d)))


RESIDUAL_CASES = [c for c in R.ALL_CASES if R.EPILOGUES[c[2]].get("residual")]


@pytest.mark.parametrize("case", RESIDUAL_CASES, ids=R.case_id)
def test_mutant_single_rounding(case):
    """Every case that carries a residual sees the double rounding: stage + final differs from one rounding of the exact value on at
    least one element (of the sampled units, for the large cases).  A case that does not gets another seed (R.SEED_BUMP)."""
    d = R.design(case)
    rows, cols = _sample(case)
    acc = R.accumulate(d, rows=rows, cols=cols)
    b, rv, res, aux = R.terms(d, rows=rows, cols=cols)
    pre = acc + (0 if b is None else b) + (0 if rv is None else rv)
    once = R.f16(pre * d["s_acc"] + d["s_res"] * res + (0 if aux is None else d["s_aux"] * aux))
    _differs(_np(once), _np(R.expected(d, rows=rows, cols=cols)))


def test_mutant_bias_of_column_n_plus_4():
    d = R.design(FULL)
    _differs(_model(d, bias=np.roll(d["bias"], -4)), _np(R.expected(d)))


def test_mutant_tail_chunk_and_row_past_m():
    d = R.design(("dense", (37, 150, 64), "bias"))
    exp = R.expected(d)
    want = R.framed(exp)
    assert want.shape == (37 + 16, 160) and R.compare(want, want, 37, 150)[:2] == (0, True)
    no_tail = want.clone()
    no_tail[:37, 144:150] = R.sentinel((37, 6))                  # the last, partial 8-column chunk never stored
    n, intact, report = R.compare(no_tail, want, 37, 150)
    assert n == 37 * 6 and intact and "(0, 144," in report
    past = want.clone()
    past[37, :150] = R.f16(torch.as_tensor(d["bias"]) * d["s_acc"])          # row M computed from a zero A row and stored
    n, intact, report = R.compare(past, want, 37, 150)
    assert n == 0 and not intact and "[37, 0]" in report
