"""The element-wise UNet kernels (csrc/norm.hip: GEGLU gate, GroupNorm [+ SiLU], LayerNorm, row softmax; gelu_pk of
csrc/common.h inside every fused gate) per element against float64.

References, tolerances (`check16`: half an fp16 ulp + a slack derived from the fp32 arithmetic) and inputs come from
tests/unet_elementwise_ref.py; tests/test_unet_elementwise_cpu.py shows without a GPU that an fp32 restatement of each kernel
meets the same tolerances on the same inputs and that subtly wrong kernels do not.  Every test records its worst err / tol."""
import numpy as np
import pytest
import torch

import unet_elementwise_ref as R

pytestmark = pytest.mark.gpu

H = torch.float16
F64 = np.float64


def dev16(a, gpu):
    """fp16 values held in a float64 array -> fp16 tensor on the GPU (exact)."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.float16))).to(gpu)


def host64(t):
    return t.detach().cpu().numpy().astype(F64)


# ---------------------------------------------------------------------------------------------- GEGLU gate
def test_geglu_every_fp16_gate(gpu, measurements):
    """ops.geglu with every finite fp16 value as a gate, against the fp32 model of the compiled polynomial and against erf in
    float64 (the bound the comment table of common.h promises)."""
    from syn3r_amd.unet import ops
    deg = R.compiled_gelu_degree()
    h, g = R.cases_gate()
    got = host64(ops.geglu(dev16(np.concatenate([h, g], axis=1), gpu)))
    assert got.shape == h.shape
    w_model, _ = R.worst16(got, R.geglu_model(h, g, deg).astype(F64), R.gate_slack_model(h, g))
    w_f64, _ = R.worst16(got, R.geglu_ref(h, g), R.gate_slack_f64(h, g, deg))
    print(f"geglu degree {deg}: err/tol {w_model:.4f} against the fp32 model, {w_f64:.4f} against float64")
    measurements("test_geglu_every_fp16_gate", degree=deg, err_over_tol_model=w_model, err_over_tol_f64=w_f64)
    R.check16(got, R.geglu_model(h, g, deg).astype(F64), R.gate_slack_model(h, g), "geglu vs fp32 model")
    R.check16(got, R.geglu_ref(h, g), R.gate_slack_f64(h, g, deg), "geglu vs float64")


def gate_matrix(D, K, gpu, row_multiple=1):
    """The gate set of `cases_gate` as the input of a fused projection + gate: x [M, K] with D hidden values in columns [0, D), their
    D gates in [D, 2 D) and zeros after; with the selection weight eye(2 D, K) and a zero bias the projection reproduces
    (hidden, gate) exactly (one product with 1, the rest with 0, summed in fp32).  Padding rows are zero (zero gates).
    Returns x, the weight, the bias and ops.geglu of the same (hidden, gate) values."""
    from syn3r_amd.unet import ops
    h, g = R.cases_gate()
    P = h.size
    M = -(-P // D)
    M = -(-M // row_multiple) * row_multiple
    hp, gp = np.zeros(M * D), np.zeros(M * D)
    hp[:P], gp[:P] = h.reshape(-1), g.reshape(-1)
    x = np.zeros((M, K))
    x[:, :D], x[:, D:2 * D] = hp.reshape(M, D), gp.reshape(M, D)
    x = dev16(x, gpu)
    w1 = torch.eye(2 * D, K, dtype=H, device=gpu)
    b1 = torch.zeros(2 * D, dtype=H, device=gpu)
    return x, w1, b1, ops.geglu(x[:, :2 * D].contiguous())


def each_contraction_kernel(body):
    """body(tile) under the per-shape default and every forced variant of syn3r_gemm_set_tile; the default is restored."""
    from syn3r_amd import _lib
    lib = _lib.load()
    try:
        for tile in (0, -128, -256, -320, -322):
            _lib.check(lib.syn3r_gemm_set_tile(tile), "set_tile")
            body(tile)
    finally:
        lib.syn3r_gemm_set_tile(0)


def test_fused_gate_linear_geglu(gpu, measurements):
    """The GEGLU epilogue of every contraction kernel == k_geglu, bit for bit, on every finite fp16 gate."""
    from syn3r_amd.unet import ops
    D, K = 32, 64
    x, w1, b1, want = gate_matrix(D, K, gpu)
    wp, bp, _ = ops.pack_geglu(w1, b1)
    differing = {}

    def body(tile):
        got = ops.linear_geglu(x, wp, bp, D)
        differing[tile] = int((got != want).sum().item())
    each_contraction_kernel(body)
    measurements("test_fused_gate_linear_geglu", differing_elements=differing)
    assert not any(differing.values()), differing


@pytest.mark.parametrize("packed64", [False, True])
def test_fused_gate_feedforward(packed64, gpu, measurements):
    """syn3r_feedforward_f16 / syn3r_feedforward_p64_f16 with selection weights in both projections: the output IS the gated hidden
    activation, bit for bit ops.geglu's."""
    from syn3r_amd import _lib
    from syn3r_amd.unet import ops
    D, K = (128, 256) if packed64 else (64, 128)
    x, w1, b1, want = gate_matrix(D, K, gpu, row_multiple=128 if packed64 else 1)
    wp, bp, _ = ops.pack_geglu(w1, b1)
    w2 = torch.eye(D, D, dtype=H, device=gpu)
    kw = {}
    if packed64:
        assert _lib.load().syn3r_feedforward_p64_supported(x.shape[0], D, K) == 1
        w64, b64, _ = ops.pack_geglu64(w1, b1)
        kw["packed64"] = (w64, b64)
    got = ops.feedforward(x, wp, bp, D, w2, None, **kw)
    bad = int((got != want).sum().item())
    measurements("test_fused_gate_feedforward", packed64=packed64, differing_elements=bad)
    assert bad == 0


def test_fused_gate_feedforward_fused_c320(gpu, measurements):
    """syn3r_feedforward_fused_f16 (C = 320, one 64-wide hidden chunk) with selection weights: bit for bit ops.geglu's.
    Its ln= form normalises the rows first, so it cannot see the same gate set: it gates what LayerNorm makes of these rows (gamma 1
    on the hidden columns, 8 on the gate columns: gates within about +-16, past the clamp on both sides) and is compared bit for
    bit with ops.geglu of ops.layernorm's output.  That rests on the fused LayerNorm being bit-equal to ops.layernorm, which
    test_unet_ops_gpu.py::test_feedforward_fused_layernorm_c320 pins."""
    from syn3r_amd.unet import ops
    D, C = 64, 320
    x, w1, b1, want = gate_matrix(D, C, gpu)
    wc, bc, _ = ops.pack_geglu_chunked(w1, b1)
    w2 = torch.eye(C, D, dtype=H, device=gpu)
    got = ops.feedforward_fused(x, wc, bc, D, w2, None)
    bad = int((got[:, :D] != want).sum().item()) + int((got[:, D:] != 0).sum().item())
    ga = torch.ones(C, dtype=H, device=gpu)
    ga[D:2 * D] = 8.0
    be = torch.zeros(C, dtype=H, device=gpu)
    n = ops.layernorm(x, ga, be)
    assert torch.isfinite(n.float()).all() and n[:, D:2 * D].float().abs().max().item() > 8.0
    want_ln = ops.geglu(n[:, :2 * D].contiguous())
    got_ln = ops.feedforward_fused(x, wc, bc, D, w2, None, ln=(ga, be, 1e-5))
    bad_ln = int((got_ln[:, :D] != want_ln).sum().item()) + int((got_ln[:, D:] != 0).sum().item())
    measurements("test_fused_gate_feedforward_fused_c320", differing_elements=bad, differing_elements_ln=bad_ln)
    assert bad == 0 and bad_ln == 0


# ---------------------------------------------------------------------------------------------- GroupNorm
def run_groupnorm(case, silu, gpu, two_source=False):
    from syn3r_amd.unet import ops
    if two_source:
        S, Rr, C1 = case["x1"].shape
        x1, x2 = dev16(case["x1"].reshape(S * Rr, C1), gpu), dev16(case["x2"].reshape(S * Rr, -1), gpu)
        out = ops.groupnorm(x1, dev16(case["gamma"], gpu), dev16(case["beta"], gpu), S, R.EPS, silu, x2=x2, use_partials=False)
    else:
        S, Rr, C = case["x"].shape
        out = ops.groupnorm(dev16(case["x"].reshape(S * Rr, C), gpu), dev16(case["gamma"], gpu), dev16(case["beta"], gpu), S, R.EPS,
                            silu, use_partials=False)
    return host64(out).reshape(S, Rr, -1)


@pytest.mark.parametrize("shape", R.GN_SHAPES, ids=str)
def test_groupnorm_shapes(shape, gpu, measurements):
    c = R.case_groupnorm(*shape)
    for silu in (False, True):
        ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], silu)
        got = run_groupnorm(c, silu, gpu)
        w, _ = R.worst16(got, ref["y"], ref["slack"])
        measurements("test_groupnorm_shapes", shape=list(shape), silu=silu, err_over_tol=w)
        R.check16(got, ref["y"], ref["slack"], f"groupnorm {shape} silu={silu}")


@pytest.mark.parametrize("C1,C2", R.GN_TWO_SOURCE)
def test_groupnorm_two_source_per_element(C1, C2, gpu, measurements):
    c = R.case_groupnorm_two_source(C1, C2)
    for silu in (False, True):
        ref = R.groupnorm_ref(c["x1"], c["gamma"], c["beta"], silu, c["x2"])
        got = run_groupnorm(c, silu, gpu, two_source=True)
        w, _ = R.worst16(got, ref["y"], ref["slack"])
        measurements("test_groupnorm_two_source_per_element", C1=C1, C2=C2, silu=silu, err_over_tol=w)
        R.check16(got, ref["y"], ref["slack"], f"groupnorm [{C1} | {C2}] silu={silu}")


def test_groupnorm_refuses_wide_rows(gpu):
    from syn3r_amd import _lib
    from syn3r_amd.unet import ops
    for C in (8200, 8224):                  # not a multiple of 32 / 1028 channel vectors for at most 1024 threads
        x = torch.zeros(8, C, dtype=H, device=gpu)
        with pytest.raises(_lib.Syn3rError):
            ops.groupnorm(x, torch.ones(C, dtype=H, device=gpu), torch.zeros(C, dtype=H, device=gpu), 1, R.EPS, False, use_partials=False)


def test_groupnorm_all_zero_group(gpu, measurements):
    """A (sample, group) of zeros: mean 0, variance 0, so the output is exactly fp16(beta) without SiLU."""
    c = R.case_groupnorm(4, 5, 320, "zero_group")
    ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"])
    got = run_groupnorm(c, False, gpu)
    w = R.check16(got, ref["y"], ref["slack"], "groupnorm with all-zero groups")
    measurements("test_groupnorm_all_zero_group", err_over_tol=w)
    assert np.array_equal(got[0, :, 30:40], np.broadcast_to(c["beta"][30:40], (5, 10)))
    assert np.array_equal(got[3, :, 310:], np.broadcast_to(c["beta"][310:], (5, 10)))
    got_silu = run_groupnorm(c, True, gpu)
    ref_silu = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], True)
    R.check16(got_silu, ref_silu["y"], ref_silu["slack"], "groupnorm + SiLU with all-zero groups")


@pytest.mark.parametrize("shape", [(4, 200, 320), (2, 9, 2560)], ids=str)
def test_groupnorm_silu_saturation(shape, gpu, measurements):
    """gamma * 64: pre-activations span about +-200, so exp(-y) overflows fp32 on one side and vanishes on the other."""
    c = R.case_groupnorm(*shape, "saturate")
    ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], True)
    got = run_groupnorm(c, True, gpu)
    w, _ = R.worst16(got, ref["y"], ref["slack"])
    measurements("test_groupnorm_silu_saturation", shape=list(shape), err_over_tol=w)
    R.check16(got, ref["y"], ref["slack"], f"groupnorm + SiLU, saturated, {shape}")


@pytest.mark.parametrize("shape", R.GN_OUTLIER_SHAPES, ids=str)
@pytest.mark.parametrize("A", R.GN_OUTLIERS)
def test_groupnorm_outlier(shape, A, gpu, measurements):
    """One value A at (row 0, first channel of a group), the rest randn: statistics that lean on one element of the group (a
    shift taken from it) lose that group's variance.  Plain slack."""
    c = R.case_groupnorm_outlier(*shape, A)
    for silu in (False, True):
        ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], silu)
        got = run_groupnorm(c, silu, gpu)
        w, _ = R.worst16(got, ref["y"], ref["slack"])
        measurements("test_groupnorm_outlier", shape=list(shape), A=A, silu=silu, err_over_tol=w)
        R.check16(got, ref["y"], ref["slack"], f"groupnorm {shape} outlier {A} silu={silu}")


@pytest.mark.parametrize("shape", R.GN_OFFSET_SHAPES, ids=str)
@pytest.mark.parametrize("off", R.GN_OFFSETS)
def test_groupnorm_offset(shape, off, gpu, measurements):
    """x = off + 0.5 randn (mean / std = 16 and 64): the one-pass statistics lose digits to the cancellation E[x^2] - mean^2.
    The slack grows by 2 allow_g, allow_g = the error of the naive left-to-right fp32 one-pass sum in that group: the kernel sums
    hierarchically and has to be at least that accurate."""
    c = R.case_groupnorm(*shape, "offset", off)
    for silu in (False, True):
        ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], silu)
        allow = R.groupnorm_offset_allowance(c, ref, silu)
        got = run_groupnorm(c, silu, gpu)
        w, _ = R.worst16(got, ref["y"], ref["slack"] + 2.0 * allow)
        w_plain, _ = R.worst16(got, ref["y"], ref["slack"])
        measurements("test_groupnorm_offset", shape=list(shape), off=off, silu=silu, err_over_tol=w, err_over_tol_without_allowance=w_plain,
                     max_allow_g=float(allow.max()))
        R.check16(got, ref["y"], ref["slack"] + 2.0 * allow, f"groupnorm {shape} off={off} silu={silu}")


@pytest.mark.parametrize("shape", R.GN_OFFSET_SHAPES, ids=str)
def test_groupnorm_offset_100_recorded(shape, gpu, measurements):
    """mean / std = 200 is a conditioning the one-pass form is not meant for: measured and recorded, not asserted (beyond a finite
    output), so that the next change of the statistics pass knows where it stands."""
    c = R.case_groupnorm(*shape, "offset", R.GN_OFFSET_RECORDED)
    for silu in (False, True):
        ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], silu)
        allow = R.groupnorm_offset_allowance(c, ref, silu)
        got = run_groupnorm(c, silu, gpu)
        assert np.all(np.isfinite(got))
        w_plain, _ = R.worst16(got, ref["y"], ref["slack"])
        w, _ = R.worst16(got, ref["y"], ref["slack"] + 2.0 * allow)
        err = np.abs(got - ref["y"])
        measurements("test_groupnorm_offset_100_recorded", shape=list(shape), silu=silu, err_over_tol_without_allowance=w_plain,
                     err_over_tol_with_2_allow_g=w, max_abs_err=float(err.max()),
                     max_allow_g=float(allow.max()))


# ---------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("C", R.LN_WIDTHS)
def test_layernorm_widths(C, gpu, measurements):
    from syn3r_amd.unet import ops
    worst = 0.0
    for M in R.LN_ROWS:
        c = R.case_layernorm(M, C)
        x, ga, be = dev16(c["x"], gpu), dev16(c["gamma"], gpu), dev16(c["beta"], gpu)
        ref = R.layernorm_ref(c["x"], c["gamma"], c["beta"])
        worst = max(worst, R.check16(host64(ops.layernorm(x, ga, be)), ref["y"], ref["slack"], f"layernorm M={M} C={C}"))
        ref = R.layernorm_ref(c["x"], c["gamma"], c["beta"], c["add"])
        y, s = ops.layernorm(x, ga, be, addvec=dev16(c["addvec"], gpu), rows_per_vec=c["rpv"], want_sum=True)
        assert np.array_equal(host64(s), ref["xsum"])                     # the fp16 sum is exact
        worst = max(worst, R.check16(host64(y), ref["y"], ref["slack"], f"layernorm + addvec M={M} C={C}"))
    measurements("test_layernorm_widths", C=C, err_over_tol=worst)


@pytest.mark.parametrize("C", R.LN_WIDTHS)
def test_layernorm_special_rows(C, gpu, measurements):
    """Constant rows (exactly fp16(beta)), a row of mean 1000 and std 1 (the two-pass variance), a row with one 65504."""
    from syn3r_amd.unet import ops
    c = R.case_layernorm_special(C)
    ref = R.layernorm_ref(c["x"], c["gamma"], c["beta"])
    got = host64(ops.layernorm(dev16(c["x"], gpu), dev16(c["gamma"], gpu), dev16(c["beta"], gpu)))
    w, _ = R.worst16(got, ref["y"], ref["slack"])
    measurements("test_layernorm_special_rows", C=C, err_over_tol=w,
                 per_row={name: R.worst16(got[i], ref["y"][i], ref["slack"][i])[0] for i, name in enumerate(R.LN_SPECIAL_ROWS)})
    R.check16(got, ref["y"], ref["slack"], f"layernorm special rows C={C}")
    assert np.array_equal(got[:2], np.broadcast_to(c["beta"], (2, C)))


def test_layernorm_refuses_wide_rows(gpu):
    from syn3r_amd import _lib
    from syn3r_amd.unet import ops
    C = 4104
    with pytest.raises(_lib.Syn3rError):
        ops.layernorm(torch.zeros(4, C, dtype=H, device=gpu), torch.ones(C, dtype=H, device=gpu), torch.zeros(C, dtype=H, device=gpu))


# ---------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("N", R.SOFTMAX_WIDTHS)
def test_softmax_rows_widths(N, gpu, measurements):
    """syn3r_softmax_rows_f16 on rows of a padded buffer (ld = 8 ceil(N / 8) + 8), out of place and in place; the padding columns
    carry a sentinel that has to survive.  N % 8 == 0: ops.softmax_rows on the dense matrix too."""
    from syn3r_amd import _lib
    from syn3r_amd.unet import ops
    lib = _lib.load()
    x64 = R.case_softmax(N)
    M, ld, hot = x64.shape[0], R.softmax_ld(N), (5 * N) // 7
    worst = 0.0

    def verify(y, scale, what):
        nonlocal worst
        ref = R.softmax_ref(x64, scale)
        worst = max(worst, R.check16(y, ref["y"], ref["slack"], what))
        assert y[2, hot] == 1.0 and np.all(np.delete(y[2], hot) == 0.0), what       # one-hot: exactly 1 and 0

    for scale in R.SOFTMAX_SCALES:
        xin = torch.full((M, ld), R.SOFTMAX_SENTINEL, dtype=H, device=gpu)
        xin[:, :N] = dev16(x64, gpu)
        before = xin.clone()
        out = torch.full((M, ld), R.SOFTMAX_SENTINEL, dtype=H, device=gpu)
        stream = _lib.stream_ptr(gpu)
        _lib.check(lib.syn3r_softmax_rows_f16(xin.data_ptr(), out.data_ptr(), M, N, ld, float(scale), stream), "softmax_rows")
        assert torch.equal(xin, before)
        assert bool((out[:, N:] == R.SOFTMAX_SENTINEL).all())
        verify(host64(out[:, :N]), scale, f"softmax N={N} scale={scale} out of place")
        _lib.check(lib.syn3r_softmax_rows_f16(xin.data_ptr(), xin.data_ptr(), M, N, ld, float(scale), stream), "softmax_rows")
        assert bool((xin[:, N:] == R.SOFTMAX_SENTINEL).all())
        assert torch.equal(xin[:, :N], out[:, :N])
        verify(host64(xin[:, :N]), scale, f"softmax N={N} scale={scale} in place")
        if N % 8 == 0:
            dense = dev16(x64, gpu)
            verify(host64(ops.softmax_rows(dense, scale)), scale, f"ops.softmax_rows N={N} scale={scale}")
            ops.softmax_rows(dense, scale, out=dense)
            verify(host64(dense), scale, f"ops.softmax_rows N={N} scale={scale} in place")
    measurements("test_softmax_rows_widths", N=N, err_over_tol=worst)
