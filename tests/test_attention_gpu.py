"""The fused attention kernels of csrc/attn.hip (k_attn_spatial, k_attn_temporal) per element.

Cases, float64 references and slacks come from tests/attention_ref.py; tests/test_attention_cpu.py shows without a GPU that a
restatement of each kernel meets the same checks on the same cases and that the flawed kernels M1-M8 do not.
  * selection designs: the output is a V row per query, compared bit for bit;
  * subset means: `check16` with slack 2^-22 |ref|;
  * numerical cases: `check16` against (a) softmax(q k^T / 8) v and against (b) the same with the kernel's prescaled fp16 operand,
    with the derived slacks.
Every test records its worst err / tol; the numerical ones record both figures and the worst error in fp16 half-ulps.

First measurement on an MI355X (no kernel change was needed): every selection case 0 differing elements; subset means err/tol
<= 0.9991 (S = 9216: the final rounding alone); spatial numerical cases <= 0.942 against (a) and <= 0.986 against (b) (both on
q 3 / k 2 and q 5 / k 2 at S = 45, where the slack is under one half-ulp); temporal <= 0.620.  The rounding of the prescaled Q
to fp16 is the largest term: on q 5 / k 2 at S = 1153 the worst element is 68 831 half-ulps from (a) and 4 809 from (b), 0.60
of what close(tol=3e-3) allows."""
import numpy as np
import pytest
import torch

import attention_ref as R
from poison import fill_bytes

pytestmark = pytest.mark.gpu

F64 = np.float64
POISON = 0x3C


def dev(a, gpu):
    return torch.from_numpy(np.array(a, np.float16, order="C")).to(gpu)          # (a copy: the cases are read-only)


def host16(t):
    return t.detach().cpu().numpy()


def differing(got, want):
    return int((np.asarray(got, np.float16).view(np.uint16) != np.asarray(want, np.float16).view(np.uint16)).sum())


def run_spatial(c, nseq, S, heads, gpu):
    from syn3r_amd.unet import ops
    out = ops.attention(dev(np.concatenate([c["q"], c["k"], c["v"]], axis=1), gpu), nseq, S, heads)
    assert out.shape == (nseq * S, heads * 64) and out.dtype == torch.float16
    return host16(out)


def run_temporal(c, shape, gpu):
    from syn3r_amd.unet import ops
    Bn, F, HW, heads = shape
    out = ops.attention_temporal(dev(np.concatenate([c["q"], c["k"], c["v"]], axis=1), gpu), Bn, F, HW, heads)
    assert out.shape == (Bn * F * HW, heads * 64) and out.dtype == torch.float16
    return host16(out)


# ---------------------------------------------------------------------------------------------- exact designs, spatial
@pytest.mark.parametrize("S", R.SELECTION_LENGTHS)
def test_selection(S, gpu, measurements):
    """out[i] == V[pi(i)] bit for bit; every (sequence, head) has its own pi and V."""
    nseq, heads = R.SPATIAL_SHAPES[S]
    wrong = {}
    for pi in R.selection_pis(S):
        c = R.case_selection(nseq, S, heads, pi)
        wrong[pi] = differing(run_spatial(c, nseq, S, heads, gpu), c["want"])
    print(f"selection S = {S} x {nseq} x {heads}: differing elements {wrong}")
    measurements(f"test_selection[{S}]", nseq=nseq, heads=heads, blocks=R.spatial_blocks(nseq, S, heads), differing_elements=wrong,
                 err_over_tol=0.0 if not any(wrong.values()) else float("inf"))
    assert not any(wrong.values()), wrong


@pytest.mark.parametrize("S", sorted(R.SUBSET_SHAPES))
def test_subset_means(S, gpu, measurements):
    """out[i] == the mean of integer V rows over subset i % 64, within half an fp16 ulp + 2^-22 |ref|."""
    nseq, heads = R.SUBSET_SHAPES[S]
    c = R.case_subsets(nseq, S, heads)
    got = run_spatial(c, nseq, S, heads, gpu).astype(F64)
    w, _ = R.worst16(got, c["want"], R.subset_slack(c["want"]))
    print(f"subset means S = {S} x {nseq} x {heads}: err/tol {w:.4f}")
    measurements(f"test_subset_means[{S}]", nseq=nseq, heads=heads, blocks=R.spatial_blocks(nseq, S, heads), err_over_tol=w)
    R.check16(got, c["want"], R.subset_slack(c["want"]), f"subset means S = {S}")


# ---------------------------------------------------------------------------------------------- numerical cases, spatial
@pytest.mark.parametrize("S", R.NUMERICAL_LENGTHS)
@pytest.mark.parametrize("kind", R.NUMERICAL_KINDS)
def test_numerical(kind, S, gpu, measurements):
    c, r = R.case_numerical(kind, S), R.refs_numerical(kind, S)
    got = run_spatial(c, 1, S, 1, gpu).astype(F64)
    wa, _ = R.worst16(got, r["ref_a"], r["slack_a"])
    wb, _ = R.worst16(got, r["ref_b"], r["slack_b"])
    hu, hu_b, old = R.half_ulps(got, r["ref_a"]), R.half_ulps(got, r["ref_b"]), R.old_close_ratio(got, r["ref_a"], 3e-3)
    print(f"{kind} S = {S}: err/tol {wa:.4f} against (a), {wb:.4f} against (b); worst error {hu:.1f} half-ulps against (a), "
          f"{hu_b:.1f} against (b); {old:.4f} of close(tol=3e-3); median slack_b {R.median_slack_ratio(r['slack_b'], r['ref_b']):.2f} "
          f"half-ulps")
    measurements(f"test_numerical[{kind}-{S}]", err_over_tol_a=wa, err_over_tol_b=wb, worst_half_ulps=hu, worst_half_ulps_b=hu_b,
                 err_over_old_close_tol=old,
                 median_slack_b_half_ulps=R.median_slack_ratio(r["slack_b"], r["ref_b"]),
                 median_slack_a_half_ulps=R.median_slack_ratio(r["slack_a"], r["ref_a"]))
    R.check16(got, r["ref_a"], r["slack_a"], f"{kind} S = {S} against (a)")
    R.check16(got, r["ref_b"], r["slack_b"], f"{kind} S = {S} against (b)")


# ---------------------------------------------------------------------------------------------- temporal kernel
@pytest.mark.parametrize("shape", R.TEMPORAL_SHAPES)
def test_temporal_exact(shape, gpu, measurements):
    wrong = {}
    for pi in R.PIS:
        c = R.case_selection_temporal(*shape, pi)
        wrong[pi] = differing(run_temporal(c, shape, gpu), c["want"])
    c = R.case_subsets_temporal(*shape)
    got = run_temporal(c, shape, gpu).astype(F64)
    w, _ = R.worst16(got, c["want"], R.subset_slack(c["want"]))
    print(f"temporal {shape}: differing elements {wrong}; subset means err/tol {w:.4f}")
    measurements(f"test_temporal_exact[{shape}]", differing_elements=wrong, err_over_tol=w)
    assert not any(wrong.values()), wrong
    R.check16(got, c["want"], R.subset_slack(c["want"]), f"temporal subset means {shape}")


@pytest.mark.parametrize("shape", R.TEMPORAL_SHAPES)
@pytest.mark.parametrize("kind", R.TEMPORAL_KINDS)
def test_temporal_numerical(kind, shape, gpu, measurements):
    c, r = R.case_numerical_temporal(kind, *shape), R.refs_numerical_temporal(kind, *shape)
    got = run_temporal(c, shape, gpu).astype(F64)
    wa, _ = R.worst16(got, r["ref_a"], r["slack_a"])
    wb, _ = R.worst16(got, r["ref_b"], r["slack_b"])
    hu, old = R.half_ulps(got, r["ref_a"]), R.old_close_ratio(got, r["ref_a"], 3e-3)
    print(f"temporal {kind} {shape}: err/tol {wa:.4f} against (a), {wb:.4f} against (b); worst error {hu:.1f} half-ulps; "
          f"{old:.4f} of close(tol=3e-3)")
    measurements(f"test_temporal_numerical[{kind}-{shape}]", err_over_tol_a=wa, err_over_tol_b=wb, worst_half_ulps=hu,
                 err_over_old_close_tol=old,
                 median_slack_b_half_ulps=R.median_slack_ratio(r["slack_b"], r["ref_b"]))
    R.check16(got, r["ref_a"], r["slack_a"], f"temporal {kind} {shape} against (a)")
    R.check16(got, r["ref_b"], r["slack_b"], f"temporal {kind} {shape} against (b)")


# ---------------------------------------------------------------------------------------------- strides, through the C entries
def strided_operands(c, rows, C, gpu):
    """q, k and v in three separate allocations [rows, 3 C + 8], each holding its operand in the columns it has in a packed q | k | v
    row and NaN everywhere else; the output [rows, C + 8] pre-filled with the poison pattern.  Returns (pointers, ld, out, ldo)."""
    ld, ldo = 3 * C + 8, C + 8
    bufs, ptrs = [], []
    for n, name in enumerate("qkv"):
        t = fill_bytes(torch.empty((rows, ld), dtype=torch.float16, device=gpu), 0xFF)
        t[:, n * C:(n + 1) * C] = dev(c[name], gpu)
        bufs.append(t)
        ptrs.append(t.data_ptr() + 2 * n * C)
    out = fill_bytes(torch.empty((rows, ldo), dtype=torch.float16, device=gpu), POISON)
    return bufs, ptrs, ld, out, ldo


def split_output(out, C):
    """(data columns [rows, C] fp16, True where every padding byte still holds the poison pattern)."""
    raw = host16(out)
    return raw[:, :C], bool(np.all(raw[:, C:].view(np.uint8) == POISON))


def test_strided_entries(gpu, measurements):
    """syn3r_attention_f16 / syn3r_attention_temporal_f16 with ld = 3 C + 8, ldo = C + 8 and q, k, v in separate allocations: one
    selection case, one subset-mean case and one temporal case; the output's padding columns keep their bytes."""
    from syn3r_amd import _lib as L
    lib = L.load()
    rec = {}

    nseq, S, heads = 2, 193, 3
    C = 64 * heads
    c = R.case_selection(nseq, S, heads, "random")
    bufs, (pq, pk, pv), ld, out, ldo = strided_operands(c, nseq * S, C, gpu)
    L.check(lib.syn3r_attention_f16(pq, pk, pv, ld, L.ptr(out), ldo, nseq, S, heads, L.stream_ptr(gpu)), "syn3r_attention_f16")
    torch.cuda.synchronize(gpu)
    got, intact = split_output(out, C)
    rec["selection_differing"] = differing(got, c["want"])
    assert intact, "selection: the output's padding columns were written"
    assert rec["selection_differing"] == 0

    nseq, S, heads = 3, 127, 5
    C = 64 * heads
    c = R.case_subsets(nseq, S, heads)
    bufs, (pq, pk, pv), ld, out, ldo = strided_operands(c, nseq * S, C, gpu)
    L.check(lib.syn3r_attention_f16(pq, pk, pv, ld, L.ptr(out), ldo, nseq, S, heads, L.stream_ptr(gpu)), "syn3r_attention_f16")
    torch.cuda.synchronize(gpu)
    got, intact = split_output(out, C)
    rec["subset_err_over_tol"], _ = R.worst16(got.astype(F64), c["want"], R.subset_slack(c["want"]))
    assert intact, "subset means: the output's padding columns were written"

    shape = (1, 25, 33, 5)
    Bn, F, HW, heads = shape
    C = 64 * heads
    ct = R.case_selection_temporal(*shape, "random")
    bufs, (pq, pk, pv), ld, out_t, ldo = strided_operands(ct, Bn * F * HW, C, gpu)
    L.check(lib.syn3r_attention_temporal_f16(pq, pk, pv, ld, L.ptr(out_t), ldo, Bn, F, HW, heads, L.stream_ptr(gpu)),
            "syn3r_attention_temporal_f16")
    torch.cuda.synchronize(gpu)
    got_t, intact_t = split_output(out_t, C)
    rec["temporal_differing"] = differing(got_t, ct["want"])
    print(f"strided entries: {rec}")
    measurements("test_strided_entries", err_over_tol=rec["subset_err_over_tol"], **rec)
    assert intact_t, "temporal: the output's padding columns were written"
    assert rec["temporal_differing"] == 0
    R.check16(got.astype(F64), c["want"], R.subset_slack(c["want"]), "strided subset means")
