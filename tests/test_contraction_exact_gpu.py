"""Every contraction kernel family of csrc/gemm.hip bit for bit against the exact-sum model of tests/contraction_ref.py.

The designs make every partial sum and every fp32 epilogue operation exact, so the expected fp16 output is known from a float64
product and two casts, whatever the tiling, the k order, the split-K association or the tap order of a kernel:
tests/test_contraction_exact_cpu.py shows that on the host, and that subtly wrong kernels do not reproduce it.
  * every assertion is `==` on fp16 values, no tolerance;
  * outputs land in sentinel-framed buffers (8+ extra columns, 16 extra rows) that must stay intact outside [M, N];
  * dense inputs, row vectors, residual and aux are column slices of wider NaN-filled buffers wherever the entry takes a stride;
  * every launch runs inside `_lib.kernel_trace()`: the tests assert that the family they mean to test ran, and record the number
    of differing elements per (case, family).

First run on an MI355X: 0 differing elements in every (case, family), every sentinel frame intact, no kernel change needed.  The
one-k-tile designs without an epilogue pass on every family, so the fp16 MFMA sums like an fp32 chain on these operands and the
1/8 x 1/16 grid stands.  Shapes the families refuse fall through to another family (the trace records which): M or N not a
multiple of 8 leave the 256 x 320 kernels, which is why TCONV_SMALL carries one M = 80 shape for k_gemm_z<2>.
"""
import pytest
import torch

import contraction_ref as R

pytestmark = pytest.mark.gpu

H = torch.float16
_SMALL = {}             # prepared operands of the small cases, shared by the tile settings of a test


def _lib():
    from syn3r_amd import _lib as L
    return L, L.load()


def up(a, gpu):
    return None if a is None else torch.as_tensor(a).to(H).contiguous().to(gpu)


def sliced(a, gpu, off=8):
    """[rows, cols] as a column slice of a wider NaN-filled buffer (row stride a multiple of 8, 16-byte aligned start)."""
    if a is None:
        return None
    rows, cols = a.shape
    buf = R.sentinel((rows, (cols + 7) // 8 * 8 + 16), gpu)
    view = buf[:, off:off + cols]
    view.copy_(torch.as_tensor(a).to(H))
    return view


def _p(t):
    return None if t is None else t.data_ptr()


def _ld(t):
    return 0 if t is None else t.stride(0)


def prepare(case, gpu):
    """Device operands of a case and its expected output in a sentinel frame (the float64 product runs on the device)."""
    if case in _SMALL:
        return _SMALL[case]
    d = R.design(case)
    M, N = d["M"], d["N"]
    t = dict(d=d, M=M, N=N, bias=up(d["bias"], gpu), rowvec=sliced(d["rowvec"], gpu), residual=sliced(d["residual"], gpu),
             aux=sliced(d["aux"], gpu), W=up(d["W"], gpu))
    if d["kind"] in ("dense", "gated"):
        t["A"] = sliced(d["A"], gpu)
    elif d["kind"] == "two_src":
        t["A1"], t["A2"] = sliced(d["A1"], gpu), sliced(d["A2"], gpu, off=16)
    else:
        t["X"] = up(d["X"], gpu)
    t["exp"] = R.expected(d, device=gpu)
    if d["kind"] != "gated":
        t["want"] = R.framed(t["exp"])
    if M * N <= 1 << 20:
        _SMALL[case] = t
    return t


def launch(t, gpu):
    """The case's C-ABI entry into a fresh sentinel-filled output buffer."""
    L, lib = _lib()
    d, M, N = t["d"], t["M"], t["N"]
    out = R.sentinel((M + R.EXTRA_ROWS, R.ldc_of(N)), gpu)
    s = L.stream_ptr(gpu)
    rv, res, aux = t["rowvec"], t["residual"], t["aux"]
    kind = d["kind"]
    if kind == "dense":
        rc = lib.syn3r_gemm_f16(_p(t["A"]), _ld(t["A"]), _p(t["W"]), _p(out), out.stride(0), _p(t["bias"]), _p(rv), _ld(rv),
                                d["rows_per_vec"], d["rv_group_rows"], _p(res), _ld(res), _p(aux), _ld(aux),
                                d["s_acc"], d["s_res"], d["s_aux"], M, N, d["K"], None, 0, None, s)
    elif kind in R.CONV_GEOM:
        stride, pad_lo, ups = R.CONV_GEOM[kind]
        NB, Hi, Wi, Cin, Cout = d["shape"]
        rc = lib.syn3r_conv2d3x3_f16(_p(t["X"]), _p(t["W"]), _p(out), out.stride(0), _p(t["bias"]), _p(rv), _ld(rv), d["rows_per_vec"],
                                     _p(res), _ld(res), d["s_acc"], d["s_res"], NB, Hi, Wi, Cin, Cout, stride, int(ups), pad_lo, None, 0, None, s)
    elif kind == "tconv":
        B, F, HW, Cin, Cout = d["shape"]
        rc = lib.syn3r_tconv3_f16(_p(t["X"]), _p(t["W"]), _p(out), out.stride(0), _p(t["bias"]), _p(rv), _ld(rv), d["rows_per_vec"],
                                  _p(res), _ld(res), d["s_acc"], d["s_res"], B, F, HW, Cin, Cout, None, 0, None, s)
    elif kind == "two_src":
        K1, K2 = d["shape"][2:]
        assert lib.syn3r_gemm_2src_supported(M, N, K1, K2, _ld(t["A1"]), _ld(t["A2"])) == 1
        rc = lib.syn3r_gemm_2src_f16(_p(t["A1"]), _ld(t["A1"]), K1, _p(t["A2"]), _ld(t["A2"]), K2, _p(t["W"]), _p(out), out.stride(0),
                                     _p(t["bias"]), M, N, None, 0, None, s)
    else:
        raise ValueError(kind)
    L.check(rc, kind)
    return out


class Tally:
    """Differing elements per (case, family) of one test; `finish` records them and fails with the collected reports."""

    def __init__(self, name):
        self.name, self.rows, self.failures, self.families = name, [], [], set()

    def add(self, case, tile, trace, n, intact, report):
        fam = sorted(k for k in trace if k.startswith("k_"))
        self.families.update(fam)
        self.rows.append([R.case_id(case), tile, fam, n])
        if n or not intact:
            self.failures.append(f"{R.case_id(case)} tile {tile} {fam}: {report}")

    def ran(self, name):
        return any(name in f for f in self.families)

    def finish(self, measurements, *wanted):
        measurements(self.name, cases=len(self.rows), differing=sum(r[3] for r in self.rows), families=sorted(self.families),
                     per_case=[r for r in self.rows if r[3]] or "0 differing in every (case, family)")
        for w in wanted:
            assert self.ran(w), (w, sorted(self.families))
        assert not self.failures, "\n".join(self.failures[:12]) + f"\n({len(self.failures)} failing (case, family) in all)"


def run_case(case, tile, gpu, tally, fn=None):
    L, lib = _lib()
    t = prepare(case, gpu)
    with L.kernel_trace() as tr:
        out = (fn or launch)(t, gpu)
        torch.cuda.synchronize()
    tally.add(case, tile, tr.result, *R.compare(out, t["want"], t["M"], t["N"]))
    return tr.result


@pytest.fixture
def set_tile():
    L, lib = _lib()

    def f(tile):
        L.check(lib.syn3r_gemm_set_tile(tile), "set_tile")
    yield f
    lib.syn3r_gemm_set_tile(0)


DENSE_FAMILY = {0: ("k_gemm_skinny", "k_gemm_dma<0,128>"), -128: ("k_gemm_dma<0,128>",), -256: ("k_gemm_dmap<0>", "k_gemm_dma<0,256>"),
                -320: ("k_gemm_widep",), -322: ("k_gemm_z<0>",)}


@pytest.mark.parametrize("tile", R.TILES)
def test_dense_every_family(tile, gpu, set_tile, measurements):
    """Every (M, N) of R.DENSE_SHAPES with 1 to 10 k-tiles and the eight epilogue variants, under every forced family."""
    tally = Tally(f"contraction_exact/dense/tile{tile}")
    set_tile(tile)
    for case in R.DENSE_SMALL:
        run_case(case, tile, gpu, tally)
    tally.finish(measurements, *DENSE_FAMILY[tile])


@pytest.mark.parametrize("K", [128, 192])
@pytest.mark.parametrize("tile,family", [(-320, "k_gemm_widep"), (-322, "k_gemm_z<0>")])
def test_persistent_wide_many_tiles(tile, family, K, gpu, set_tile, measurements):
    """9 x 31 tiles of 256 x 320 on the persistent kernels: ragged last row tile, 8-column last band, even and odd k-tile counts."""
    tally = Tally(f"contraction_exact/wide_many/tile{tile}/K{K}")
    set_tile(tile)
    for case in R.DENSE_WIDE_MANY:
        if case[1][2] == K:
            assert family in "".join(run_case(case, tile, gpu, tally))
    tally.finish(measurements, family)


def test_persistent_dmap_many_tiles(gpu, set_tile, measurements):
    tally = Tally("contraction_exact/dmap_many")
    set_tile(-256)
    for case in R.DENSE_DMAP_MANY:
        assert "k_gemm_dmap<0>" in "".join(run_case(case, -256, gpu, tally))
    tally.finish(measurements, "k_gemm_dmap<0>")


@pytest.mark.parametrize("case", R.DENSE_DMAPD, ids=R.case_id)
def test_deferred_epilogue_kernel(case, gpu, measurements):
    """k_gemm_dmapd by default dispatch (264 whole 256 x 160 tiles), with and without a residual, both row-vector indexings."""
    tally = Tally(f"contraction_exact/dmapd/{R.case_id(case)}")
    assert "k_gemm_dmapd" in "".join(run_case(case, 0, gpu, tally))
    tally.finish(measurements, "k_gemm_dmapd")


@pytest.mark.parametrize("tile,family", [(0, "k_gemm_widep"), (-320, "k_gemm_widep"), (-322, "k_gemm_z<0>")])
def test_two_source(tile, family, gpu, set_tile, measurements):
    """[A1 | A2] read in place (strided sources), K1 / K2 of one to three k-tiles, and 279 tiles on 256 CUs."""
    tally = Tally(f"contraction_exact/two_src/tile{tile}")
    set_tile(tile)
    for case in R.TWO_SRC:
        assert family in "".join(run_case(case, tile, gpu, tally))
    tally.finish(measurements, family)


def test_skinny(gpu, measurements):
    """k_gemm_skinny<2 | 8 | 16>: K split over the lanes at a 512-element stride (K = 64: most lanes idle; 1280: a ragged last
    round), two columns per wavefront (N = 161: the one-column last wavefront), s_acc = 0.5 with the bias."""
    tally = Tally("contraction_exact/skinny")
    for case in R.SKINNY:
        names = "".join(run_case(case, 0, gpu, tally))
        M = case[1][0]
        assert f"k_gemm_skinny<{2 if M <= 2 else 8 if M <= 8 else 16}>" in names, (case, names)
    tally.finish(measurements, "k_gemm_skinny<2>", "k_gemm_skinny<8>", "k_gemm_skinny<16>")


CONV_FAMILY = {0: ("k_gemm_",), -128: ("k_gemm_dma<1,128>",), -256: ("k_gemm_dma<1,256>",), -322: ("k_gemm_z<1>",)}


@pytest.mark.parametrize("tile", [0, -128, -256, -322])
def test_conv3x3(tile, gpu, set_tile, measurements):
    """Stride 1, stride 2 with pad_lo 1 and 0, the fused nearest-2x upsample, per-image row vector + residual."""
    tally = Tally(f"contraction_exact/conv/tile{tile}")
    set_tile(tile)
    for case in R.CONV_SMALL:
        run_case(case, tile, gpu, tally)
    tally.finish(measurements, *CONV_FAMILY[tile])


@pytest.mark.parametrize("case", R.CONV_MANY, ids=R.case_id)
def test_conv3x3_many_tiles(case, gpu, set_tile, measurements):
    """k_gemm_z<1> with 279 tiles on 256 CUs: the cross-tile prefetch on a convolution, with and without the upsample."""
    tally = Tally(f"contraction_exact/conv_many/{R.case_id(case)}")
    set_tile(-322)
    assert "k_gemm_z<1>" in "".join(run_case(case, -322, gpu, tally))
    tally.finish(measurements, "k_gemm_z<1>")


def _up4(t, gpu):
    from syn3r_amd.unet import ops
    L, lib = _lib()
    NB, Hi, Wi, Cin, Cout = t["d"]["shape"]
    w4 = ops.pack_upsample4(t["W"])
    out = R.sentinel((t["M"] + R.EXTRA_ROWS, Cout), gpu)                     # dense rows: only the rows past M frame it
    L.check(lib.syn3r_conv2d3x3_up4_f16(_p(t["X"]), _p(w4), _p(out), _p(t["bias"]), None, NB, Hi, Wi, Cin, Cout, None, 0, None,
                                        L.stream_ptr(gpu)), "up4")
    return out


@pytest.mark.parametrize("case", R.UP4, ids=R.case_id)
def test_conv3x3_up4(case, gpu, measurements):
    """The four-phase form on folded weights (sums of at most four 1/16-grid weights: exact in fp16) gives the bits of
    conv3x3(upsample=True)."""
    L, lib = _lib()
    tally = Tally(f"contraction_exact/up4/{R.case_id(case)}")
    t = prepare(case, gpu)
    with L.kernel_trace() as tr:
        out = _up4(t, gpu)
        torch.cuda.synchronize()
    want = R.framed(t["exp"], ldc=t["N"])
    tally.add(case, 0, tr.result, *R.compare(out, want, t["M"], t["N"]))
    tally.finish(measurements, "/up4")


TCONV_FAMILY = {0: ("k_gemm_",), -128: ("k_gemm_dma<2,128>",), -256: ("k_gemm_dmap<2>",), -322: ("k_gemm_z<2>",)}


@pytest.mark.parametrize("tile", [0, -128, -256, -322])
def test_tconv3(tile, gpu, set_tile, measurements):
    tally = Tally(f"contraction_exact/tconv/tile{tile}")
    set_tile(tile)
    for case in R.TCONV_SMALL:
        run_case(case, tile, gpu, tally)
    tally.finish(measurements, *TCONV_FAMILY[tile])


def test_tconv3_frame_minor_many_tiles(gpu, set_tile, measurements):
    """HW = 256: k_gemm_dmap<2> walks its 372 tiles with the frame index minor (tc_pb, tc_nf)."""
    tally = Tally("contraction_exact/tconv_many")
    set_tile(-256)
    for case in R.TCONV_MANY:
        assert "k_gemm_dmap<2>" in "".join(run_case(case, -256, gpu, tally))
    tally.finish(measurements, "k_gemm_dmap<2>")


@pytest.mark.parametrize("case,parts", R.SPLITK, ids=lambda v: R.case_id(v) if isinstance(v, tuple) else str(v))
def test_split_k(case, parts, gpu, measurements):
    """Two and four K parts + k_splitk_finish: the same bits as one pass, because every partial sum is exact."""
    L, lib = _lib()
    tally = Tally(f"contraction_exact/splitk/{R.case_id(case)}")
    t = prepare(case, gpu)
    ws = torch.empty(4 * t["M"] * t["N"] * 4, dtype=torch.uint8, device=gpu)
    try:
        L.check(lib.syn3r_gemm_set_splitk_workspace(ws.data_ptr(), ws.numel()), "set_splitk")
        with L.kernel_trace(detail=True) as tr:
            out = launch(t, gpu)
            torch.cuda.synchronize()
    finally:
        lib.syn3r_gemm_set_splitk_workspace(None, 0)
    tally.add(case, 0, tr.result, *R.compare(out, t["want"], t["M"], t["N"]))
    assert any(f"256>/{parts}" in k for k in tr.result), list(tr.result)
    tally.finish(measurements, "k_splitk_finish")


# ------------------------------------------------------------------------------------------------------- gated projections
def _gated(case, gpu):
    """Packed operands of a gated case and the expected gate output: ops.geglu of the model's fp16 projection [hidden | gate]."""
    from syn3r_amd.unet import ops
    t = prepare(case, gpu)
    if "gate" not in t:
        t["gate"] = ops.geglu(t["exp"].contiguous())
    return t


def _count(got, want):
    return int((~(got == want)).sum())


def _report(got, want):
    bad = (~(got == want)).nonzero()[:6].cpu()
    return [(int(m), int(n), float(got[m, n]), float(want[m, n])) for m, n in bad]


@pytest.mark.parametrize("tile", R.TILES)
def test_linear_geglu(tile, gpu, set_tile, measurements):
    from syn3r_amd.unet import ops
    L, lib = _lib()
    tally = Tally(f"contraction_exact/geglu/tile{tile}")
    set_tile(tile)
    for case in R.GEGLU_SMALL + (R.GEGLU_MANY if tile in (-320, -322) else []):
        t = _gated(case, gpu)
        M, D, K = case[1]
        if "wp" not in t:
            t["wp"], t["bp"], _ = ops.pack_geglu(t["W"], t["bias"])
        out = R.sentinel((M + R.EXTRA_ROWS, R.ldc_of(D)), gpu)
        with L.kernel_trace() as tr:
            L.check(lib.syn3r_gemm_geglu_f16(_p(t["A"]), _ld(t["A"]), _p(t["wp"]), _p(t["bp"]), _p(out), out.stride(0), M, D, K, L.stream_ptr(gpu)), "geglu")
            torch.cuda.synchronize()
        tally.add(case, tile, tr.result, *R.compare(out, R.framed(t["gate"]), M, D))
        if case in R.GEGLU_MANY:
            assert ("k_gemm_widep" if tile == -320 else "k_gemm_z<0>") in "".join(tr.result), list(tr.result)
    tally.finish(measurements, *{0: (), -128: ("k_gemm_dma<0,128>",), -256: ("k_gemm_dma<0,256>",), -320: ("k_gemm_widep",), -322: ("k_gemm_z<0>",)}[tile])


def _ff_cases(cases, gpu, tally, tile, family, packed64=False):
    from syn3r_amd.unet import ops
    L, lib = _lib()
    for case in cases:
        t = _gated(case, gpu)
        M, D, K = case[1]
        x = up(t["d"]["A"], gpu)
        wp, bp, _ = ops.pack_geglu(t["W"], t["bias"])
        kw = dict(packed64=ops.pack_geglu64(t["W"], t["bias"])[:2]) if packed64 else {}
        eye = torch.eye(D, dtype=H, device=gpu)
        with L.kernel_trace() as tr:
            out = ops.feedforward(x, wp, bp, D, eye, **kw)
            torch.cuda.synchronize()
        n = _count(out, t["gate"])
        tally.add(case, tile, tr.result, n, True, _report(out, t["gate"]) if n else "")
        assert family in "".join(tr.result), list(tr.result)


@pytest.mark.parametrize("tile", R.TILES)
def test_feedforward_hidden_activation(tile, gpu, set_tile, measurements):
    """w2 = I: the output is the gated hidden activation read back out of the A-tiled workspace by net.2."""
    tally = Tally(f"contraction_exact/ff/tile{tile}")
    set_tile(tile)
    _ff_cases(R.FF_PLAIN, gpu, tally, tile, "k_gemm_")
    tally.finish(measurements)


@pytest.mark.parametrize("case", R.FF_P64, ids=R.case_id)
def test_feedforward_g256(case, gpu, measurements):
    """k_gemm_g256: one tile, a half last row tile (M = 384), 2 and 5 k-tiles, and 280 tiles on 256 CUs (M = 2432: half last row tile)."""
    tally = Tally(f"contraction_exact/g256/{R.case_id(case)}")
    _ff_cases([case], gpu, tally, 0, "k_gemm_g256", packed64=True)
    tally.finish(measurements, "k_gemm_g256")


@pytest.mark.parametrize("case", R.FF_FUSED, ids=R.case_id)
def test_feedforward_fused(case, gpu, measurements):
    """k_ffn320r with w2 selecting one 320-wide block of the hidden activation per call."""
    from syn3r_amd.unet import ops
    L, lib = _lib()
    tally = Tally(f"contraction_exact/ffn320/{R.case_id(case)}")
    t = _gated(case, gpu)
    M, D, K = case[1]
    x = sliced(t["d"]["A"], gpu)
    wc, bc, _ = ops.pack_geglu_chunked(t["W"], t["bias"])
    for off in range(0, D, 320):
        w = min(320, D - off)
        w2 = torch.zeros((320, D), dtype=H, device=gpu)
        i = torch.arange(w, device=gpu)
        w2[i, off + i] = 1
        want = torch.zeros((M, 320), dtype=H, device=gpu)
        want[:, :w] = t["gate"][:, off:off + w]
        with L.kernel_trace() as tr:
            out = ops.feedforward_fused(x, wc, bc, D, w2)
            torch.cuda.synchronize()
        n = _count(out, want)
        tally.add(case, off, tr.result, n, True, _report(out, want) if n else "")
    tally.finish(measurements, "k_gemm_ffn320")
