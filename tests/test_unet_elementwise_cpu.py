"""CPU side of the per-element tests of the element-wise UNet kernels (tests/unet_elementwise_ref.py).

Three things are established here, without a GPU, before tests/test_unet_elementwise_gpu.py applies the same tolerances to the
HIP kernels:
  * the polynomial tables of gelu_pk (csrc/common.h), all four degrees, keep the error bound their comment table prints;
  * FEASIBILITY: on every case the GPU file runs, a plain fp32 restatement of the kernel passes `check16` with the same slack,
    so a failure on the GPU is the kernel's and not the tolerance's;
  * TEETH: subtly wrong kernels (NumPy mutants) fail `check16` - and, where stated, pass the `close()` metric of
    tests/test_unet_ops_gpu.py, which is the record of the gap the per-element comparison closes.
"""
import numpy as np
import pytest

import unet_elementwise_ref as R

F64 = np.float64


# ---------------------------------------------------------------------------------------------- the comparison itself
def test_ulp16_and_check16():
    assert R.ulp16(1.0) == 2.0 ** -10 and R.ulp16(1.999) == 2.0 ** -10 and R.ulp16(2.0) == 2.0 ** -9
    assert R.ulp16(0.0) == 2.0 ** -24 and R.ulp16(2.0 ** -14) == 2.0 ** -24 and R.ulp16(2.0 ** -13) == 2.0 ** -23
    assert R.ulp16(65504.0) == 32.0
    v = R.all_finite_f16()
    assert v.size == 63488
    pos = np.sort(v[v > 0])
    assert np.array_equal(np.diff(pos), R.ulp16(pos[:-1]))               # the spacing of fp16 itself
    ref = np.array([1.0 + 2.0 ** -12, 3.0, 1e-9])
    assert R.check16(R.f16(ref), ref, 0.0) <= 1.0                        # correct rounding always passes with no slack
    with pytest.raises(AssertionError):
        R.check16(np.array([1.0 + 2.0 ** -10]), np.array([1.0]), 0.0)    # one whole ulp does not
    with pytest.raises(AssertionError):
        R.check16(np.array([1.0, np.nan]), np.array([1.0, 1.0]), 0.0)
    with pytest.raises(AssertionError):
        R.check16(np.array([np.inf]), np.array([70000.0]), 0.0)


# ---------------------------------------------------------------------------------------------- GELU tables
def test_gelu_header_parse():
    tables, default = R.parse_gelu_tables()
    assert sorted(tables) == [8, 9, 10, 12] and default in tables
    for deg, t in tables.items():
        assert t["c"].size == deg + 1 and t["c"].dtype == np.float32
        assert abs(float(t["SC"]) - 2.0 / float(t["G"]) ** 2) < 1e-7        # t = 2 g^2 / G^2 - 1
    printed = {12: 2.3e-6, 10: 2.6e-5, 9: 3.7e-5, 8: 6.3e-5}
    unit = {12: 1e-7, 10: 1e-6, 9: 1e-6, 8: 1e-6}
    for deg in printed:
        assert tables[deg]["E"] == pytest.approx(printed[deg] + 0.5 * unit[deg], rel=1e-12)


@pytest.mark.parametrize("deg", [8, 9, 10, 12])
def test_gelu_table_meets_its_bound(deg):
    """The fp32 model of gelu_pk over ALL finite fp16 gates against erf in float64: within the table's bound for |g| <= 8 and
    within |g| (Phi(-G) + E / G) past it."""
    g = R.all_finite_f16()
    err = np.abs(R.gelu_pk_model(g, deg).astype(F64) - R.gelu64(g))
    bound = R.gelu_bound(g, deg) + 2.0 ** -20 * np.abs(g)                # + the model's own fp32 roundings
    worst = float((err / bound).max())
    inner = float(err[np.abs(g) <= 8.0].max())
    print(f"degree {deg}: max |error| for |g| <= 8 = {inner:.4g}, worst err / bound = {worst:.4f}")
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------- feasibility
def test_feasible_gate():
    h, g = R.cases_gate()
    assert np.all(np.isfinite(g)) and np.abs(h * g).max() <= 65504.0
    for r in range(h.shape[0]):
        if abs(h[r, 0]) <= 1.0:                                          # full rows: every finite fp16 value is a gate
            assert np.array_equal(np.sort(g[r]), np.sort(R.all_finite_f16()))
    assert np.abs(g[3]).max() == 20000.0 and np.abs(g[5]).max() == 60.0
    ref = R.geglu_ref(h, g)
    for deg in (8, 9, 10, 12):
        got = R.f16(R.geglu_model(h, g, deg))
        w = R.check16(got, ref, R.gate_slack_f64(h, g, deg), f"gate model deg {deg} vs float64")
        print(f"degree {deg}: model vs float64 err/tol = {w:.4f}")


def _gn_feasible(case, silu, x2=None, extra=None):
    x = case["x"] if x2 is None else case["x1"]
    ref = R.groupnorm_ref(x, case["gamma"], case["beta"], silu, x2)
    got = R.f16(R.groupnorm_model(x, case["gamma"], case["beta"], silu, x2))
    slack = ref["slack"] if extra is None else ref["slack"] + extra(ref)
    return R.check16(got, ref["y"], slack, "groupnorm model")


@pytest.mark.parametrize("shape", R.GN_SHAPES, ids=str)
@pytest.mark.parametrize("silu", [False, True])
def test_feasible_groupnorm(shape, silu):
    _gn_feasible(R.case_groupnorm(*shape), silu)


@pytest.mark.parametrize("C1,C2", R.GN_TWO_SOURCE)
def test_feasible_groupnorm_two_source(C1, C2):
    c = R.case_groupnorm_two_source(C1, C2)
    for silu in (False, True):
        _gn_feasible(c, silu, x2=c["x2"])


def test_feasible_groupnorm_zero_group_and_saturation():
    c = R.case_groupnorm(4, 5, 320, "zero_group")
    ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"])
    got = R.f16(R.groupnorm_model(c["x"], c["gamma"], c["beta"]))
    R.check16(got, ref["y"], ref["slack"], "zero group")
    assert np.array_equal(got[0, :, 30:40], np.broadcast_to(c["beta"][30:40], (5, 10)))     # exactly fp16(beta)
    assert np.array_equal(ref["y"][0, :, 30:40], np.broadcast_to(c["beta"][30:40], (5, 10)))
    for shape in ((4, 200, 320), (2, 9, 2560)):
        c = R.case_groupnorm(*shape, "saturate")
        ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], True)
        assert ref["pre"].min() < -150 and ref["pre"].max() > 150
        _gn_feasible(c, True)


@pytest.mark.parametrize("shape", R.GN_OFFSET_SHAPES, ids=str)
@pytest.mark.parametrize("off", R.GN_OFFSETS + (R.GN_OFFSET_RECORDED,))
def test_feasible_groupnorm_offset(shape, off):
    """x = off + 0.5 randn: the naive one-pass model is within the slack + 2 allow_g by construction (allow_g is its own error);
    what this records is how much of the tolerance the plain slack leaves to the statistics."""
    c = R.case_groupnorm(*shape, "offset", off)
    for silu in (False, True):
        ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], silu)
        allow = R.groupnorm_offset_allowance(c, ref, silu)
        got = R.f16(R.groupnorm_model(c["x"], c["gamma"], c["beta"], silu))
        w = R.check16(got, ref["y"], ref["slack"] + 2.0 * allow, "offset groupnorm model")
        w0, _ = R.worst16(got, ref["y"], ref["slack"])
        print(f"{shape} off={off} silu={silu}: naive model err/tol = {w:.3f} with 2 allow_g, {w0:.3f} without; "
              f"max allow_g = {allow.max():.3g}")


@pytest.mark.parametrize("shape", R.GN_OFFSET_SHAPES, ids=str)
@pytest.mark.parametrize("off", R.GN_OFFSETS + (R.GN_OFFSET_RECORDED,))
def test_merged_statistics_need_no_allowance(shape, off):
    """The form k_gn_stats uses (per-thread shifted squares -> M2, merged pairwise) in fp32 meets the PLAIN slack at every offset
    (mean / std up to 200), where the naive one-pass sum is 3 to 1600 times outside it (test_feasible_groupnorm_offset's
    records)."""
    c = R.case_groupnorm(*shape, "offset", off)
    for silu in (False, True):
        ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], silu)
        R.check16(R.f16(R.groupnorm_model(c["x"], c["gamma"], c["beta"], silu, merged=True)), ref["y"], ref["slack"], "merged model")


@pytest.mark.parametrize("shape", [sh for sh in R.GN_SHAPES if sh[0] < 100], ids=str)
def test_merged_statistics_feasible_on_the_plain_cases(shape):
    c = R.case_groupnorm(*shape)
    for silu in (False, True):
        ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], silu)
        for rows in (1, 8):
            got = R.groupnorm_model(c["x"], c["gamma"], c["beta"], silu, merged=True, thread_rows=rows)
            R.check16(R.f16(got), ref["y"], ref["slack"], f"merged model, {rows} rows per thread")


@pytest.mark.parametrize("shape", R.GN_OUTLIER_SHAPES, ids=str)
@pytest.mark.parametrize("A", R.GN_OUTLIERS)
def test_feasible_groupnorm_outlier(shape, A):
    """One value A at (row 0, first channel of a group): the naive form and the merged form both meet the plain slack; a single
    shift K = that element does not (teeth: the variance E[(x - K)^2] - (mean - K)^2 cancels A^2 against 1)."""
    c = R.case_groupnorm_outlier(*shape, A)
    for silu in (False, True):
        ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], silu)
        for merged in (False, True):
            got = R.groupnorm_model(c["x"], c["gamma"], c["beta"], silu, merged=merged)
            R.check16(R.f16(got), ref["y"], ref["slack"], f"outlier {A}, merged={merged}")
    # the mutant: one shift per group, K = x[row 0, first channel]
    x = c["x"].astype(np.float32)
    S, Rr, C = x.shape
    cpg = C // 32
    xg = x.reshape(S, Rr, 32, cpg).transpose(0, 2, 1, 3).reshape(S, 32, -1)
    k = xg[:, :, :1]
    n = np.float32(xg.shape[2])
    m = xg.sum(axis=2, dtype=np.float32) / n
    var = np.maximum(((xg - k) ** 2).sum(axis=2, dtype=np.float32) / n - (m - k[:, :, 0]) ** 2, np.float32(0))
    rstd = np.repeat(1.0 / np.sqrt(var + np.float32(R.EPS)), cpg, axis=1).astype(np.float32)
    mean = np.repeat(m, cpg, axis=1)
    g32, b32 = c["gamma"].astype(np.float32), c["beta"].astype(np.float32)
    bad = x * (rstd * g32)[:, None, :] + (b32 - mean * rstd * g32)[:, None, :]
    ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"])
    w, _ = R.worst16(R.f16(bad), ref["y"], ref["slack"])
    assert w > 1.0, w


@pytest.mark.parametrize("C", R.LN_WIDTHS)
def test_feasible_layernorm(C):
    for M in R.LN_ROWS:
        c = R.case_layernorm(M, C)
        for add in (None, c["add"]):
            ref = R.layernorm_ref(c["x"], c["gamma"], c["beta"], add)
            R.check16(R.f16(R.layernorm_model(c["x"], c["gamma"], c["beta"], add)), ref["y"], ref["slack"], f"layernorm model M={M}")
    c = R.case_layernorm_special(C)
    ref = R.layernorm_ref(c["x"], c["gamma"], c["beta"])
    got = R.f16(R.layernorm_model(c["x"], c["gamma"], c["beta"]))
    R.check16(got, ref["y"], ref["slack"], "layernorm model, special rows")
    assert np.array_equal(got[:2], np.broadcast_to(c["beta"], (2, C))) and np.array_equal(ref["y"][:2], got[:2])
    assert abs(c["x"][2].mean() - 1000.0) < 1.5 and 0.3 < c["x"][2].std() < 2.5       # 8 to 4096 samples of mean 1000, std 1


@pytest.mark.parametrize("N", R.SOFTMAX_WIDTHS)
def test_feasible_softmax(N):
    x = R.case_softmax(N)
    for scale in R.SOFTMAX_SCALES:
        ref = R.softmax_ref(x, scale)
        got = R.f16(R.softmax_model(x, scale))
        R.check16(got, ref["y"], ref["slack"], f"softmax model N={N} scale={scale}")
        hot = (5 * N) // 7
        assert got[2, hot] == 1.0 and np.all(np.delete(got[2], hot) == 0.0)
        assert ref["y"][2, hot] == 1.0 and np.all(np.delete(ref["y"][2], hot) == 0.0)


# ---------------------------------------------------------------------------------------------- teeth
def test_teeth_gate_top_coefficient_dropped():
    """Degree 8 with a wrong top coefficient c[8] = 1.829e-3, on the old test's input distribution (randn * 2, [333, 2 * 640]).
    Phi is off by dc t^8 gc, the gate by h g gc dc t^8 (t^8 = 1 past the clamp, which 3 % of these gates are).
      * c[8] with one digit mistyped (1.629e-3, dc = 2e-4): max error ~0.04, PASSES the old metric (2e-3 max|ref| + 1e-3 = 0.09)
        and fails the per-element comparison many times over;
      * c[8] dropped (dc = 1.8e-3): max error 0.38 - four times the old tolerance, so the old test does see this one (a gate
        error of 1.8e-3 would pass it; a Phi error of 1.8e-3 is multiplied by |h g| <= 45) - and fails the per-element comparison
        here and on the full gate set, against float64 and against the fp32 model."""
    t = R.parse_gelu_tables()[0][8]
    cut = np.concatenate([t["c"][:-1], np.zeros(1, np.float32)])
    typo = np.concatenate([t["c"][:-1], np.array([1.629005353e-03], np.float32)])
    assert abs(float(t["c"][-1]) - 1.829005353e-03) < 1e-9
    rng = np.random.default_rng(2)
    x = R.f16(rng.standard_normal((333, 2 * 640)) * 2.0)
    h, g = x[:, :640], x[:, 640:]
    ref = R.geglu_ref(h, g)
    assert R.check16(R.f16(R.geglu_model(h, g, 8)), ref, R.gate_slack_f64(h, g, 8)) <= 1.0
    for name, coeffs, old_passes in (("with one digit mistyped", typo, True), ("dropped", cut, False)):
        bad = R.f16(R.geglu_model(h, g, 8, coeffs))
        err = np.abs(bad - ref).max()
        assert R.old_close(bad, ref) == old_passes, (name, err)
        w, _ = R.worst16(bad, ref, R.gate_slack_f64(h, g, 8))
        assert w > 1.0
        print(f"top coefficient {name}: max error {err:.3g} against close()'s {2e-3 * np.abs(ref).max() + 1e-3:.3g}; "
              f"err/tol = {w:.1f} under check16")
    h, g = R.cases_gate()
    w, _ = R.worst16(R.f16(R.geglu_model(h, g, 8, cut)), R.geglu_ref(h, g), R.gate_slack_f64(h, g, 8))
    assert w > 1.0
    wm, _ = R.worst16(R.f16(R.geglu_model(h, g, 8, cut)), R.geglu_model(h, g, 8).astype(F64), R.gate_slack_model(h, g))
    assert wm > 1.0


def test_teeth_groupnorm_groups_per_vector():
    """Groups assigned per 8-channel vector (the group of the vector's first channel) instead of per channel: C = 320 has 10
    channels per group, so every vector that straddles two groups is normalised with the wrong statistics."""
    C = 320
    c = R.case_groupnorm(4, 200, C)
    wrong = ((np.arange(C) // 8) * 8) // (C // 32)
    assert np.any(wrong != np.arange(C) // (C // 32))
    for silu in (False, True):
        ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], silu)
        w, _ = R.worst16(R.f16(R.groupnorm_model(c["x"], c["gamma"], c["beta"], silu, group_of=wrong)), ref["y"], ref["slack"])
        assert w > 1.0


@pytest.mark.parametrize("silu", [False, True])
def test_teeth_groupnorm_rstd_off(silu):
    """rstd off by 2e-3 relative (what one-pass statistics lose at mean / std ~ 200): inside the old tolerance, outside the new."""
    c = R.case_groupnorm(4, 200, 320)
    ref = R.groupnorm_ref(c["x"], c["gamma"], c["beta"], silu)
    bad = R.f16(R.groupnorm_model(c["x"], c["gamma"], c["beta"], silu, rstd_scale=1.002))
    assert R.old_close(bad, ref["y"], tol=3e-3)
    w, _ = R.worst16(bad, ref["y"], ref["slack"])
    assert w > 1.0
    print(f"rstd * 1.002: max error {np.abs(bad - ref['y']).max():.3g} passes close(tol=3e-3), err/tol = {w:.1f} under check16")


@pytest.mark.parametrize("N", [n for n in R.SOFTMAX_WIDTHS if n % 8])
def test_teeth_softmax_tail_left_out_of_the_sum(N):
    x = R.case_softmax(N)
    ref = R.softmax_ref(x, 1.0)
    bad = R.softmax_model(x, 1.0, sum_upto=N - N % 8)
    bad = np.where(np.isfinite(bad), bad, 65504.0 * 2)                   # N < 8: an empty sum, not a number
    w, _ = R.worst16(R.f16(np.minimum(bad, 65504.0)), ref["y"], ref["slack"])
    assert w > 1.0
    w_equal, _ = R.worst16(R.f16(np.minimum(bad, 65504.0))[1], ref["y"][1], ref["slack"][1])    # the all-equal row alone
    assert w_equal > 1.0


@pytest.mark.parametrize("C", [200, 328, 1288])
def test_teeth_layernorm_padded_width(C):
    """Statistics divided by the padded width.  Every admitted C is a multiple of 8, so 8 * ceil(C / 8) == C changes nothing;
    the padding a LayerNorm bug can actually pick up is the lane layout's (8 * LPR * ceil(C / 8 / LPR) channels: a dropped
    `cv < cvec` guard), which differs from C at the ragged widths."""
    padded = R.ln_lane_padded_width(C)
    assert 8 * -(-C // 8) == C and padded > C and R.ln_lane_padded_width(320) == 320
    c = R.case_layernorm(33, C)
    ref = R.layernorm_ref(c["x"], c["gamma"], c["beta"])
    w, _ = R.worst16(R.f16(R.layernorm_model(c["x"], c["gamma"], c["beta"], divide_by=padded)), ref["y"], ref["slack"])
    assert w > 1.0
