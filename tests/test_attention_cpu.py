"""CPU side of the per-element tests of the fused attention kernels (tests/attention_ref.py; csrc/attn.hip).

Established here, without a GPU, before tests/test_attention_gpu.py applies the same checks to the HIP kernels:
  * CONDITIONS: the exact designs are what they claim (logits 0 / <= -128, non-empty subsets, outputs inside fp16), the shapes
    cover every grid remainder of xcd_remap and leave wavefronts without an item, and on the peaked cases the derived slack is a
    few half-ulps (printed for the diffuse ones, where a worst-case sum over many keys is loose by nature);
  * FEASIBILITY: on every case the GPU file runs, the fp32 / fp16 restatement of the kernel meets exactly the check the GPU file
    applies (bit equality, `check16` with 2^-22 |ref|, `check16` against both float64 references);
  * TEETH: each of the flawed kernels M1-M8 fails one of those checks on one of those cases; whether `close(tol=3e-3)` of
    tests/test_unet_ops_gpu.py would have passed the same output is printed next to it.
"""
import numpy as np
import pytest

import attention_ref as R

F64 = np.float64


def spatial_args(c):
    return c["q"], c["k"], c["v"]


# ---------------------------------------------------------------------------------------------- conditions
def test_layouts_round_trip():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((2 * 7, 3 * 64))
    assert np.array_equal(R.spatial_pack(R.spatial_unpack(a, 2, 7, 3), 2, 7, 3), a)
    blk = R.spatial_unpack(a, 2, 7, 3)
    assert np.array_equal(blk[1 * 3 + 2], a[7:14, 128:192])                       # sequence 1, head 2
    b = rng.standard_normal((2 * 5 * 3, 2 * 64))
    assert np.array_equal(R.temporal_pack(R.temporal_unpack(b, 2, 5, 3, 2), 2, 5, 3, 2), b)
    blk = R.temporal_unpack(b, 2, 5, 3, 2)                                        # item (b = 1, pix = 2, head = 1), frame 4
    assert np.array_equal(blk[(1 * 3 + 2) * 2 + 1][4], b[(1 * 5 + 4) * 3 + 2, 64:128])


def test_selection_design_logits():
    """Key pi(i) has logit exactly 0, every other key -128 or -256; the prescaled operand keeps them below exp2's fp32 range."""
    for S in (1, 2, 33, 65, 700, 1024):
        for pi in R.PIS:
            p = R.make_pi(pi, S, 0, 0)
            q, k, v, want = R.selection_block(S, p, np.random.default_rng(0))
            for a in (q, k, v):
                assert a.dtype == np.float16 and np.all(np.isfinite(a))
            logit = q.astype(F64) @ k.astype(F64).T / 8.0
            assert np.all(logit[np.arange(S), p] == 0.0)
            others = np.ones((S, S), bool)
            others[np.arange(S), p] = False
            assert set(np.unique(logit[others])) <= {-128.0, -256.0}
            qt = (q.astype(np.float32) * R.C_PRESCALE).astype(np.float16).astype(F64)
            assert (qt @ k.astype(F64).T)[others].max(initial=-200.0) < -150.0      # exp2 flushes below -149
            assert np.array_equal(want, v[p])
    assert np.array_equal(R.make_pi("identity", 9, 0, 0), np.arange(9)) and np.array_equal(R.make_pi("last", 9, 0, 0), np.full(9, 8))
    assert not np.array_equal(R.make_pi("random", 65, 0, 0), R.make_pi("random", 65, 1, 0))


@pytest.mark.parametrize("S", sorted(R.SUBSET_SHAPES))
def test_subset_design(S):
    nseq, heads = R.SUBSET_SHAPES[S]
    c = R.case_subsets(nseq, S, heads)
    assert c["sizes"].min() >= 1                                                  # every subset is non-empty
    assert np.abs(c["want"]).max() <= 8.0                                         # no expected output leaves the fp16 range
    m = R.make_subsets(S, 0, 0)
    assert m[0].all() and m[1].sum() == 1 and m[1][-1] and m[2].sum() == 1 and m[2][0]
    assert S == 1 or (m[3].sum() == S - 1 and not m[3][-1])
    assert m[4].sum() == S - 64 * ((S - 1) // 64) and m[4][-1] and m[5].sum() == min(S, 64)
    assert S < 64 or m[6].sum() == S // 64
    assert m[7].sum() == (S + 1) // 2
    q, k = c["q"].astype(F64), c["k"].astype(F64)
    assert set(np.unique(k)) <= {0.0, -R.B} and set(np.unique(q)) <= {0.0, R.A}


def test_shapes_cover_the_grid():
    counts = {R.spatial_blocks(nseq, S, heads) for S, (nseq, heads) in R.SUBSET_SHAPES.items()}
    assert {n % 8 for n in counts} == set(range(8)) and {1, 7, 9} <= counts
    counts_sel = {R.spatial_blocks(nseq, S, heads) for S, (nseq, heads) in R.SPATIAL_SHAPES.items()}
    assert {0, 1, 2, 3, 4, 6, 7} <= {n % 8 for n in counts_sel}
    assert set(R.SPATIAL_SHAPES.values()) == {(1, 1), (2, 3), (3, 5)}
    for Bn, F, HW, heads in R.TEMPORAL_SHAPES:
        assert (Bn * HW * heads) % 4 != 0 and 1 <= F <= 32
    assert {s[1] for s in R.TEMPORAL_SHAPES} == {1, 2, 7, 14, 16, 17, 25, 31, 32}
    assert {s[2] for s in R.TEMPORAL_SHAPES} == {1, 33} and {s[3] for s in R.TEMPORAL_SHAPES} == {1, 5}


# ---------------------------------------------------------------------------------------------- feasibility: exact designs
@pytest.mark.parametrize("S", R.SELECTION_LENGTHS)
def test_feasible_selection(S):
    nseq, heads = R.SPATIAL_SHAPES[S]
    for pi in R.selection_pis(S):
        c = R.case_selection(nseq, S, heads, pi)
        got = R.spatial_model(*spatial_args(c), nseq, S, heads)
        assert np.array_equal(got.view(np.uint16), c["want"].view(np.uint16)), (S, pi)
    print(f"selection S = {S} x {nseq} x {heads}: {len(R.selection_pis(S))} maps exact")


@pytest.mark.parametrize("S", sorted(R.SUBSET_SHAPES))
def test_feasible_subsets(S):
    nseq, heads = R.SUBSET_SHAPES[S]
    c = R.case_subsets(nseq, S, heads)
    got = R.spatial_model(*spatial_args(c), nseq, S, heads)
    w = R.check16(got, c["want"], R.subset_slack(c["want"]), f"subset means S = {S}")
    print(f"subset means S = {S} x {nseq} x {heads}: err/tol {w:.4f}")


@pytest.mark.parametrize("shape", R.TEMPORAL_SHAPES)
def test_feasible_exact_temporal(shape):
    for pi in R.PIS:
        c = R.case_selection_temporal(*shape, pi)
        got = R.temporal_model(*spatial_args(c), *shape)
        assert np.array_equal(got.view(np.uint16), c["want"].view(np.uint16)), (shape, pi)
    c = R.case_subsets_temporal(*shape)
    assert c["sizes"].min() >= 1 and np.abs(c["want"]).max() <= 8.0
    got = R.temporal_model(*spatial_args(c), *shape)
    w = R.check16(got, c["want"], R.subset_slack(c["want"]), f"temporal subset means {shape}")
    print(f"temporal {shape}: {len(R.PIS)} maps exact, subset means err/tol {w:.4f}")


# ---------------------------------------------------------------------------------------------- feasibility: numerical cases
@pytest.mark.parametrize("S", R.NUMERICAL_LENGTHS)
@pytest.mark.parametrize("kind", R.NUMERICAL_KINDS)
def test_feasible_numerical(kind, S):
    c, r = R.case_numerical(kind, S), R.refs_numerical(kind, S)
    got = R.spatial_model_block(*spatial_args(c)).astype(F64)
    ratio = R.median_slack_ratio(r["slack_b"], r["ref_b"])
    wa, _ = R.worst16(got, r["ref_a"], r["slack_a"])
    wb, _ = R.worst16(got, r["ref_b"], r["slack_b"])
    print(f"{kind} S = {S}: err/tol {wa:.4f} against (a), {wb:.4f} against (b); median slack_b = {ratio:.2f} half-ulps "
          f"(slack_a {R.median_slack_ratio(r['slack_a'], r['ref_a']):.1f}); worst error {R.half_ulps(got, r['ref_a']):.1f} half-ulps; "
          f"close(3e-3) {R.old_close(got, r['ref_a'], 3e-3)}")
    assert np.abs(r["ref_a"]).max() + r["slack_a"].max() < 65504.0
    R.check16(got, r["ref_a"], r["slack_a"], f"{kind} S = {S} against (a)")
    R.check16(got, r["ref_b"], r["slack_b"], f"{kind} S = {S} against (b)")
    if kind in R.PEAKED_KINDS:
        assert ratio <= 8.0, "the slack would hide whole ulps on a peaked case"


@pytest.mark.parametrize("shape", R.TEMPORAL_SHAPES)
@pytest.mark.parametrize("kind", R.TEMPORAL_KINDS)
def test_feasible_numerical_temporal(kind, shape):
    c, r = R.case_numerical_temporal(kind, *shape), R.refs_numerical_temporal(kind, *shape)
    got = R.temporal_model(*spatial_args(c), *shape).astype(F64)
    ratio = R.median_slack_ratio(r["slack_b"], r["ref_b"])
    wa, _ = R.worst16(got, r["ref_a"], r["slack_a"])
    wb, _ = R.worst16(got, r["ref_b"], r["slack_b"])
    print(f"temporal {kind} {shape}: err/tol {wa:.4f} against (a), {wb:.4f} against (b); median slack_b = {ratio:.2f} half-ulps; "
          f"worst error {R.half_ulps(got, r['ref_a']):.1f} half-ulps")
    R.check16(got, r["ref_a"], r["slack_a"], f"temporal {kind} {shape} against (a)")
    R.check16(got, r["ref_b"], r["slack_b"], f"temporal {kind} {shape} against (b)")
    if kind == "peaked_4_2":
        assert ratio <= 8.0


# ---------------------------------------------------------------------------------------------- teeth
def _passes(fn):
    try:
        fn()
        return True
    except AssertionError:
        return False


def verdict_selection(S, pi, mutant):
    nseq, heads = R.SPATIAL_SHAPES[S]
    c = R.case_selection(nseq, S, heads, pi)
    got = R.spatial_model(*spatial_args(c), nseq, S, heads, mutant=mutant)
    return np.array_equal(got.view(np.uint16), c["want"].view(np.uint16)), R.old_close(got, c["want"], 3e-3)


def verdict_subsets(S, mutant):
    nseq, heads = R.SUBSET_SHAPES[S]
    c = R.case_subsets(nseq, S, heads)
    got = R.spatial_model(*spatial_args(c), nseq, S, heads, mutant=mutant)
    return _passes(lambda: R.check16(got, c["want"], R.subset_slack(c["want"]))), R.old_close(got, c["want"], 3e-3)


def verdict_numerical(kind, S, mutant):
    c, r = R.case_numerical(kind, S), R.refs_numerical(kind, S)
    got = R.spatial_model_block(*spatial_args(c), mutant=mutant).astype(F64)
    ok = _passes(lambda: (R.check16(got, r["ref_a"], r["slack_a"]), R.check16(got, r["ref_b"], r["slack_b"])))
    return ok, R.old_close(got, r["ref_a"], 3e-3)


def verdict_selection_temporal(shape, pi, mutant):
    c = R.case_selection_temporal(*shape, pi)
    got = R.temporal_model(*spatial_args(c), *shape, mutant=mutant)
    return np.array_equal(got.view(np.uint16), c["want"].view(np.uint16)), R.old_close(got, c["want"], 3e-3)


def verdict_subsets_temporal(shape, mutant):
    c = R.case_subsets_temporal(*shape)
    got = R.temporal_model(*spatial_args(c), *shape, mutant=mutant)
    return _passes(lambda: R.check16(got, c["want"], R.subset_slack(c["want"]))), R.old_close(got, c["want"], 3e-3)


def verdict_numerical_temporal(kind, shape, mutant):
    c, r = R.case_numerical_temporal(kind, *shape), R.refs_numerical_temporal(kind, *shape)
    got = R.temporal_model(*spatial_args(c), *shape, mutant=mutant).astype(F64)
    ok = _passes(lambda: (R.check16(got, r["ref_a"], r["slack_a"]), R.check16(got, r["ref_b"], r["slack_b"])))
    return ok, R.old_close(got, r["ref_a"], 3e-3)


# mutant -> the cases of the GPU file it is tried on: (name, verdict function, arguments)
MUTANT_CASES = {
    "M1": [("selection identity S = 33", verdict_selection, (33, "identity")),
           ("subset means S = 65", verdict_subsets, (65,)),
           ("peaked_3_2 S = 130", verdict_numerical, ("peaked_3_2", 130))],
    "M2": [("selection identity S = 65", verdict_selection, (65, "identity")),
           ("subset means S = 65", verdict_subsets, (65,)),
           ("subset means S = 700", verdict_subsets, (700,))],
    "M3": [("selection last S = 129", verdict_selection, (129, "last")),
           ("subset means S = 129", verdict_subsets, (129,)),
           ("growth_12 S = 700", verdict_numerical, ("growth_12", 700))],
    "M4": [("subset means S = 9216", verdict_subsets, (9216,))],
    "M5": [("selection random S = 129", verdict_selection, (129, "random")),
           ("peaked_5_2 S = 130", verdict_numerical, ("peaked_5_2", 130)),
           ("peaked_4_2 S = 1153", verdict_numerical, ("peaked_4_2", 1153)),
           ("randn S = 130", verdict_numerical, ("randn", 130)),
           ("temporal peaked_4_2 (1, 25, 1, 5)", verdict_numerical_temporal, ("peaked_4_2", (1, 25, 1, 5)))],
    "M6": [("temporal selection last (2, 7, 1, 5)", verdict_selection_temporal, ((2, 7, 1, 5), "last")),
           ("temporal subset means (1, 17, 33, 1)", verdict_subsets_temporal, ((1, 17, 33, 1),)),
           ("temporal subset means (1, 32, 33, 5)", verdict_subsets_temporal, ((1, 32, 33, 5),)),
           ("temporal randn (2, 7, 1, 5)", verdict_numerical_temporal, ("randn", (2, 7, 1, 5)))],
    "M7": [("selection random S = 65 (2 x 3 heads)", verdict_selection, (65, "random")),
           ("selection identity S = 64 (1 x 1 head)", verdict_selection, (64, "identity")),
           ("temporal selection identity (2, 7, 1, 5)", verdict_selection_temporal, ((2, 7, 1, 5), "identity"))],
    "M8": [("selection identity S = 193", verdict_selection, (193, "identity")),
           ("selection identity S = 257", verdict_selection, (257, "identity")),
           ("subset means S = 257", verdict_subsets, (257,)),
           ("randn S = 700", verdict_numerical, ("randn", 700))],
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_fails_a_gpu_check(mutant):
    failed = []
    for name, verdict, args in MUTANT_CASES[mutant]:
        assert verdict(*args, None)[0], f"the unflawed restatement fails {name}"
        ok, old = verdict(*args, mutant)
        print(f"{mutant} on {name}: new check {'passes' if ok else 'FAILS'}; close(tol=3e-3) {'passes' if old else 'fails'}")
        if not ok:
            failed.append(name)
    assert failed, f"{mutant} passes every check it was tried on"
