"""float64 references, fp32 models, derived tolerances and shared cases for the element-wise UNet kernels
(csrc/norm.hip: GEGLU gate, GroupNorm [+ SiLU], LayerNorm, row softmax; csrc/common.h: gelu_pk).

Plain NumPy, no device code: tests/test_unet_elementwise_cpu.py shows on the CPU that every tolerance is reachable by an fp32
restatement of the kernel and that it rejects subtly wrong kernels; tests/test_unet_elementwise_gpu.py feeds the same cases
to the HIP kernels.

The comparison is per element: |got - ref| <= half an fp16 ulp of the result + `slack`, where `slack` bounds what fp32
arithmetic may lose BEFORE the result is rounded to fp16.  Every slack below is derived from the arithmetic; none is fitted
to what a kernel returns.
"""
from __future__ import annotations

import math
import re
from functools import lru_cache
from pathlib import Path

import numpy as np

F32 = np.float32
F64 = np.float64
COMMON_H = Path(__file__).resolve().parents[1] / "syn3r_amd" / "csrc" / "common.h"
EPS = 1e-5
F16_MAX = 65504.0


# ------------------------------------------------------------------------------------------------ the comparison
def ulp16(v):
    """Spacing of fp16 at magnitude v: 2^(floor(log2 v) - 10) for v >= 2^-14, 2^-24 (the subnormal spacing) below."""
    v = np.maximum(np.abs(np.asarray(v, F64)), 2.0 ** -14)
    _, e = np.frexp(v)                       # v = m * 2^e, m in [0.5, 1): floor(log2 v) = e - 1
    return np.ldexp(1.0, e - 1 - 10)


def tol16(ref, slack):
    ref = np.asarray(ref, F64)
    slack = np.broadcast_to(np.asarray(slack, F64), ref.shape)
    return 0.5 * ulp16(np.abs(ref) + slack) + slack


def worst16(got, ref, slack):
    """max(err / tol) over every element, and its flat index (no assertion)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ratio = np.abs(got - ref) / tol16(ref, slack)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    i = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[i]), i


def check16(got, ref, slack, what=""):
    """Assert |got - ref| <= 0.5 * ulp16(|ref| + slack) + slack for EVERY element; returns max(err / tol)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert np.all(np.abs(ref) + np.asarray(slack, F64) < 65520.0), f"{what}: an expected output leaves the fp16 range"
    w, i = worst16(got, ref, slack)
    assert w <= 1.0, (f"{what}: err/tol = {w:.4g} at flat index {i} of shape {got.shape}: got {got.reshape(-1)[i]!r}, "
                      f"ref {ref.reshape(-1)[i]!r}, tol {tol16(ref, slack).reshape(-1)[i]:.4g}")
    return w


def f16(a):
    """Round to fp16 (nearest even, subnormals kept) and return as float64."""
    return np.asarray(a).astype(np.float16).astype(F64)


def old_close(got, ref, tol=2e-3):
    """The metric of tests/test_unet_ops_gpu.py (`close`): ONE comparison of the largest error with the largest output."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return bool(np.abs(got - ref).max() <= tol * (np.abs(ref).max() + 1e-6) + 1e-3)


# ------------------------------------------------------------------------------------------------ GELU gate
_erfc = np.frompyfunc(math.erfc, 1, 1)


def phi64(g):
    """Standard normal CDF in float64 (erfc: no cancellation in the lower tail)."""
    g = np.asarray(g, F64)
    return 0.5 * np.asarray(_erfc(-g / math.sqrt(2.0)), F64)


def gelu64(g):
    g = np.asarray(g, F64)
    return g * phi64(g)


def geglu_ref(h, g):
    return np.asarray(h, F64) * gelu64(g)


@lru_cache(maxsize=None)
def parse_gelu_tables():
    """{degree: dict(G, SC, c = fp32 coefficients, E = printed |error| bound + half a unit of its last digit)} and the default
    degree, read from csrc/common.h: the four `#if / #elif SYN3R_GELU_DEG ==` blocks of gelu_pk and its comment table."""
    text = COMMON_H.read_text()
    num = r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?"
    tables = {}
    blocks = re.split(r"#(?:el)?if SYN3R_GELU_DEG == (\d+)", text)
    for deg, body in zip(blocks[1::2], blocks[2::2]):
        body = re.split(r"#(?:elif|else|endif)", body)[0]
        G = re.search(rf"\bG = ({num})f", body)
        SC = re.search(rf"\bSC = ({num})f", body)
        cm = re.search(r"c\[(\d+)\] = \{([^}]*)\}", body)
        assert G and SC and cm, f"gelu_pk degree {deg}: G / SC / c[] not found"
        c = [F32(v) for v in re.findall(rf"({num})f", cm.group(2))]
        assert int(cm.group(1)) == len(c)
        tables[int(deg)] = dict(G=F32(G.group(1)), SC=F32(SC.group(1)), c=np.array(c, F32))
    for m in re.finditer(r"//\s+SYN3R_GELU_DEG (\d+)\b.*?\|error\| <= (\d+)\.(\d+)e(-\d+)", text):
        deg, ip, fp, ex = int(m.group(1)), m.group(2), m.group(3), int(m.group(4))
        printed = float(f"{ip}.{fp}e{ex}")
        tables[deg]["E"] = printed + 0.5 * 10.0 ** (ex - len(fp))
    default = int(re.search(r"#ifndef SYN3R_GELU_DEG\s*\n#define SYN3R_GELU_DEG (\d+)", text).group(1))
    return tables, default


def compiled_gelu_degree():
    return parse_gelu_tables()[1]


def gelu_pk_model(g, deg, coeffs=None):
    """gelu_pk of csrc/common.h in NumPy float32, operation for operation (no fused multiply-add: see `gate_slack_model`)."""
    t_ = parse_gelu_tables()[0][deg]
    G, SC = t_["G"], t_["SC"]
    c = t_["c"] if coeffs is None else np.asarray(coeffs, F32)
    g = np.asarray(g, F32)
    gc = np.clip(g, -G, G)
    t = gc * gc * SC - F32(1.0)
    a = t * c[-1] + c[-2]
    for k in range(len(c) - 3, -1, -1):
        a = a * t + c[k]
    return g * (gc * a + F32(0.5))


def geglu_model(h, g, deg, coeffs=None):
    return np.asarray(h, F32) * gelu_pk_model(g, deg, coeffs)


def gate_slack_model(h, g):
    """Kernel against the fp32 model: 2^-20 |h g| = at most 16 fp32 roundings (the model rounds after every operation, the
    kernel once per fused multiply-add) of terms bounded by |h g|, since |gc a + 1/2| <= 1."""
    return 2.0 ** -20 * np.abs(np.asarray(h, F64) * np.asarray(g, F64))


def gelu_bound(g, deg):
    """E(g): the bound on |gelu_pk(g) - gelu64(g)| that the comment table of common.h promises.  |g| <= 8: the printed figure
    (+ half a unit of its last digit).  Beyond: the kernel's Phi is the constant Phi_k(G) of the clamp; by the table at g = G it
    is within E / G of Phi64(G), and Phi64 moves by at most 1 - Phi64(G) = Phi64(-G) after that."""
    t_ = parse_gelu_tables()[0][deg]
    E, G = t_["E"], float(t_["G"])
    ag = np.abs(np.asarray(g, F64))
    return np.where(ag <= 8.0, E, ag * (float(phi64(-G)) + E / G))


def gate_slack_f64(h, g, deg):
    return np.abs(np.asarray(h, F64)) * gelu_bound(g, deg) + gate_slack_model(h, g)


def all_finite_f16():
    """Every finite fp16 value once (63 488 of them, both zeros and the subnormals included), as float64."""
    v = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    return v[np.isfinite(v)].astype(F64)


GATE_HIDDEN = (1.0, -1.0, float(np.float16(1.0 / 3.0)), 3.0, 2.0 ** -10, 1000.0)
GATE_CEILING = 60000.0     # |hidden * gate| kept below this: 1000 * 60 (and 3 * 20000), so no expected output leaves fp16


@lru_cache(maxsize=None)
def cases_gate():
    """(hidden, gate), both [6, 63488] float64 holding fp16 values: every finite fp16 value as a gate, one hidden value per row.
    Gates whose product with the row's hidden value would pass GATE_CEILING are replaced by 0 (the 1000 row keeps |g| <= 60, the
    3 row |g| <= 20000; the other rows keep everything: gelu(65504) = 65504 is still an fp16 number)."""
    gates = all_finite_f16()
    h = np.repeat(np.array(GATE_HIDDEN, F64)[:, None], gates.size, 1)
    g = np.repeat(gates[None, :], len(GATE_HIDDEN), 0)
    g = np.where((np.abs(h) <= 1.0) | (np.abs(h * g) <= GATE_CEILING), g, 0.0)
    h.setflags(write=False)
    g.setflags(write=False)
    return h, g


# ------------------------------------------------------------------------------------------------ norms
def silu64(y):
    y = np.asarray(y, F64)
    with np.errstate(over="ignore"):
        return y / (1.0 + np.exp(-y))


def norm_slack(x, xhat, mean, rstd, gamma, beta):
    """2^-16 (|gamma x_hat| + |beta|) + 2^-21 (|x| + |mean|) rstd |gamma|.
    First term: rsqrt, v_exp, v_rcp and two fused roundings are a few 2^-23 relative each, below 2^-19 together; 2^-16 leaves 8x
    over that and is still 32x under one fp16 ulp, so an indexing or statistics bug moves an element by whole ulps.
    Second term: x and mean are rounded to fp32 (2^-24 relative each, several times) before they cancel."""
    return 2.0 ** -16 * (np.abs(gamma * xhat) + np.abs(beta)) + 2.0 ** -21 * (np.abs(x) + np.abs(mean)) * rstd * np.abs(gamma)


def groupnorm_ref(x, gamma, beta, silu=False, x2=None, eps=EPS):
    """x [samples, rows, C] (x2 [samples, rows, C2]: the channel concatenation [x | x2] is normalised), 32 groups, biased variance.
    Returns dict(y, pre, xhat, mean, rstd, slack): mean / rstd broadcast to y's shape, slack = the norm slack, the same with and
    without SiLU (its 2^-16 term counts v_exp and v_rcp)."""
    x = np.asarray(x, F64)
    if x2 is not None:
        x = np.concatenate([x, np.asarray(x2, F64)], axis=2)
    S, R, C = x.shape
    gamma, beta = np.asarray(gamma, F64), np.asarray(beta, F64)
    xg = x.reshape(S, R, 32, C // 32)
    mean = xg.mean(axis=(1, 3), keepdims=True)
    var = ((xg - mean) ** 2).mean(axis=(1, 3), keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = ((xg - mean) * rstd).reshape(S, R, C)
    mean = np.broadcast_to(mean, xg.shape).reshape(S, R, C)
    rstd = np.broadcast_to(rstd, xg.shape).reshape(S, R, C)
    pre = gamma * xhat + beta
    slack = norm_slack(x, xhat, mean, rstd, gamma, beta)
    y = pre
    if silu:
        y = silu64(pre)
    return dict(y=y, pre=pre, xhat=xhat, mean=mean, rstd=rstd, slack=slack)


def _seq_sum32(a, axis=-1):
    """Left-to-right fp32 sum (np.cumsum accumulates sequentially; np.sum would add pairwise)."""
    a = np.asarray(a, F32)
    if a.shape[axis] == 0:
        return np.zeros(np.delete(a.shape, axis), F32)
    return np.take(np.cumsum(a, axis=axis, dtype=F32), -1, axis=axis)


def _merge_stats(n, s, m2):
    """Pairwise tree over the last axis of (count, sum, M2) triples in fp32: M2 += M2b + (mean_b - mean_a)^2 na nb / (na + nb)."""
    while n.shape[-1] > 1:
        if n.shape[-1] % 2:
            n, s, m2 = (np.concatenate([a, np.zeros(a.shape[:-1] + (1,), F32)], axis=-1) for a in (n, s, m2))
        (na, nb), (sa, sb), (ma, mb) = ((a[..., 0::2], a[..., 1::2]) for a in (n, s, m2))
        tot = na + nb
        with np.errstate(divide="ignore", invalid="ignore"):
            mean_a = np.where(na > 0, sa / na, F32(0.0)).astype(F32)
            mean_b = np.where(nb > 0, sb / nb, F32(0.0)).astype(F32)
            w = np.where(tot > 0, na * (nb / tot), F32(0.0)).astype(F32)
        delta = np.where((na > 0) & (nb > 0), mean_b - mean_a, F32(0.0)).astype(F32)
        n, s, m2 = tot, sa + sb, ma + mb + delta * delta * w
    return n[..., 0], s[..., 0], m2[..., 0]


def groupnorm_model(x, gamma, beta, silu=False, x2=None, eps=EPS, group_of=None, rstd_scale=1.0, merged=False, thread_rows=8):
    """GroupNorm in fp32, then the kernel's apply: a = rstd gamma, b = beta - mean rstd gamma, y = x a + b.
    Default: the NAIVE one-pass form, left-to-right sums of x and x^2 over the whole group (rows outermost),
    var = E[x^2] - mean^2 clamped at 0.
    merged: the form of k_gn_stats / k_gn_finalize - per channel and run of `thread_rows` rows ("a thread"), the sums of x and of
    (x - K)^2 with K = the run's first value, turned into M2 = sum (x - K)^2 - n (mean - K)^2; the (count, sum, M2) triples of a
    group merged pairwise (a tree here; the kernel's fixed order differs, its arithmetic does not); mean = sum / n, var = M2 / n.
    group_of (channel -> group) and rstd_scale are for the mutants of the CPU test (naive form only)."""
    x = np.asarray(x, F32)
    if x2 is not None:
        x = np.concatenate([x, np.asarray(x2, F32)], axis=2)
    S, R, C = x.shape
    cpg = C // 32
    gamma, beta = np.asarray(gamma, F32), np.asarray(beta, F32)
    mean, rstd = np.zeros((S, C), F32), np.zeros((S, C), F32)
    if merged:
        assert group_of is None
        ns, ss, ms = [], [], []
        for r0 in range(0, R, thread_rows):
            xb = x[:, r0:r0 + thread_rows]                                  # [S, n, C]
            n = F32(xb.shape[1])
            k = xb[:, :1]
            d = xb - k
            s1, q = _seq_sum32(xb, 1), _seq_sum32(d * d, 1)
            dm = s1 / n - k[:, 0]
            ns.append(np.full_like(s1, n))
            ss.append(s1)
            ms.append(np.maximum(q - n * dm * dm, F32(0.0)))
        grouped = lambda a: np.stack(a, axis=1).reshape(S, -1, 32, cpg).transpose(0, 2, 1, 3).reshape(S, 32, -1)
        n, s1, m2 = _merge_stats(grouped(ns), grouped(ss), grouped(ms))
        inv_n = F32(1.0) / n
        mean[:] = np.repeat(s1 * inv_n, cpg, axis=1)
        rstd[:] = np.repeat(F32(1.0) / np.sqrt(np.maximum(m2 * inv_n, F32(0.0)) + F32(eps)), cpg, axis=1)
    else:
        grp = np.arange(C) // cpg if group_of is None else np.asarray(group_of)
        for g in range(32):
            sel = grp == g
            n = int(sel.sum()) * R
            if n == 0:
                continue
            xs = x[:, :, sel].reshape(S, -1)
            s1, s2 = _seq_sum32(xs), _seq_sum32(xs * xs)
            inv_n = F32(1.0) / F32(n)
            m = s1 * inv_n
            var = np.maximum(s2 * inv_n - m * m, F32(0.0))
            mean[:, sel] = m[:, None]
            rstd[:, sel] = (F32(1.0) / np.sqrt(var + F32(eps)))[:, None] * F32(rstd_scale)
    a = rstd * gamma
    b = beta - mean * rstd * gamma
    y = x * a[:, None, :] + b[:, None, :]
    if silu:
        with np.errstate(over="ignore"):
            y = y * (F32(1.0) / (F32(1.0) + np.exp(-y)))
    return y


def layernorm_ref(x, gamma, beta, add=None, eps=EPS):
    """x [M, C]; add [M, C] (already expanded per row) is added in fp16 first, as the kernel and the tensor add it replaces do.
    Returns dict(y, xsum, xhat, mean, rstd, slack)."""
    x = np.asarray(x, F64)
    if add is not None:
        x = f16(x + np.asarray(add, F64))          # the exact sum of two fp16 numbers, rounded once: the fp16 add
    gamma, beta = np.asarray(gamma, F64), np.asarray(beta, F64)
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean) * rstd
    y = gamma * xhat + beta
    return dict(y=y, xsum=x, xhat=xhat, mean=mean, rstd=rstd, slack=norm_slack(x, xhat, mean, rstd, gamma, beta))


def layernorm_model(x, gamma, beta, add=None, eps=EPS, divide_by=None):
    """Two-pass LayerNorm in fp32: left-to-right sum, mean, left-to-right sum of squared deviations.
    divide_by: the width the statistics are divided by (the mutant of the CPU test)."""
    x = np.asarray(x, F64)
    if add is not None:
        x = f16(x + np.asarray(add, F64))
    x = x.astype(F32)
    C = F32(x.shape[1] if divide_by is None else divide_by)
    mean = (_seq_sum32(x, 1) / C)[:, None]
    d = x - mean
    rstd = (F32(1.0) / np.sqrt(_seq_sum32(d * d, 1) / C + F32(eps)))[:, None]
    return d * rstd * np.asarray(gamma, F32) + np.asarray(beta, F32)


def ln_lane_padded_width(C):
    """Channels a row occupies in k_layernorm's lane layout: LPR lanes x ceil(cvec / LPR) vectors of 8 (launcher's LPR choice)."""
    cvec, lpr = C // 8, 8
    while lpr < 64 and (cvec + lpr - 1) // lpr > 5:
        lpr *= 2
    return 8 * lpr * ((cvec + lpr - 1) // lpr)


# ------------------------------------------------------------------------------------------------ softmax
def softmax_ref(x, scale):
    """x [M, N].  Returns dict(y, slack): slack = y (2^-16 + 2^-22 (|x scale| + |max scale|)); the second part is the rounding of
    the exponent's argument (the product, the difference and the base-2 conversion: <= 4 roundings of 2^-24 of its two terms)."""
    x = np.asarray(x, F64) * scale
    mx = x.max(axis=1, keepdims=True)
    e = np.exp(x - mx)
    y = e / e.sum(axis=1, keepdims=True)
    return dict(y=y, slack=y * (2.0 ** -16 + 2.0 ** -22 * (np.abs(x) + np.abs(mx))))


def softmax_model(x, scale, sum_upto=None):
    """The three loops of k_softmax_rows in fp32: max, sum of exp(x scale - max scale), exp(...) / sum.
    sum_upto: only the first `sum_upto` columns enter the sum (the mutant of the CPU test)."""
    x = np.asarray(x, F32)
    scale = F32(scale)
    mx = x.max(axis=1, keepdims=True) * scale
    e = np.exp(x * scale - mx)
    s = _seq_sum32(e if sum_upto is None else e[:, :sum_upto], 1)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return e * (F32(1.0) / s)


# ------------------------------------------------------------------------------------------------ shared cases
def _randn16(rng, *shape, scale=1.0, shift=0.0):
    return f16(rng.standard_normal(shape) * scale + shift)


# (samples, rows, C): one row, rows < 8, one chunk per sample with long per-thread loops (2100 samples), groups that straddle the
# 8-channel vectors (C = 320: 10 channels per group; 960: 30; 1920: 60), rows-per-block == 1 (C >= 2048), the 1024-thread limit
GN_SHAPES = ((1, 1, 32), (3, 7, 32), (2100, 40, 32), (4, 5, 320), (4, 200, 320), (2, 257, 320), (2, 64, 960), (2, 33, 1920),
             (2, 9, 2560), (1, 8, 8192))
GN_TWO_SOURCE = ((8, 24), (320, 320), (640, 320), (320, 640))          # (C1, C2); 640 + 320: a group of 30 straddles the sources
GN_OFFSET_SHAPES = ((4, 200, 320), (2, 77, 2560))
GN_OFFSETS = (8.0, 32.0)
GN_OFFSET_RECORDED = 100.0                                             # measured, not asserted


@lru_cache(maxsize=None)
def case_groupnorm(samples, rows, C, kind="randn", offset=0.0):
    """dict(x [samples, rows, C], gamma, beta) of fp16 values (float64 arrays), fixed seed.
    kind: 'randn'; 'zero_group' (sample 0's group 3 and the last sample's last group all zero); 'saturate' (gamma * 64);
    'offset' (x = offset + 0.5 randn)."""
    rng = np.random.default_rng([samples, rows, C, int(offset), ("randn", "zero_group", "saturate", "offset").index(kind)])
    if kind == "offset":
        x = _randn16(rng, samples, rows, C, scale=0.5, shift=offset)
    else:
        x = _randn16(rng, samples, rows, C)
    gamma, beta = _randn16(rng, C), _randn16(rng, C)
    if kind == "saturate":
        gamma = f16(gamma * 64.0)
    if kind == "zero_group":
        cpg = C // 32
        x[0, :, 3 * cpg:4 * cpg] = 0.0
        x[-1, :, 31 * cpg:] = 0.0
    for a in (x, gamma, beta):
        a.setflags(write=False)
    return dict(x=x, gamma=gamma, beta=beta)


GN_OUTLIER_SHAPES = ((1, 4096, 320), (2, 77, 2560))
GN_OUTLIERS = (100.0, 1000.0)


@lru_cache(maxsize=None)
def case_groupnorm_outlier(samples, rows, C, A):
    """randn with ONE value A per sample at row 0 (the corner pixel), first channel of a group: group 0 in sample 0, group 5 in the
    last sample.  Statistics that lean on that one element (as a shift, say) lose the variance of its whole group."""
    c = case_groupnorm(samples, rows, C)
    x = c["x"].copy()
    x[0, 0, 0] = A
    x[-1, 0, 5 * (C // 32)] = A
    x.setflags(write=False)
    return dict(x=x, gamma=c["gamma"], beta=c["beta"])


@lru_cache(maxsize=None)
def case_groupnorm_two_source(C1, C2, samples=2, rows=37):
    c = case_groupnorm(samples, rows, C1 + C2)
    return dict(x1=np.ascontiguousarray(c["x"][:, :, :C1]), x2=np.ascontiguousarray(c["x"][:, :, C1:]), gamma=c["gamma"], beta=c["beta"])


def groupnorm_offset_allowance(case, ref, silu):
    """allow_g of the offset cases: per (sample, group), the largest |y_naive - ref| of the naive fp32 one-pass model, broadcast to
    every element of the group.  The kernel sums hierarchically (per thread, per block, a tree over the blocks), so its
    statistics are at least as accurate as the left-to-right sum's; the caller adds TWICE this to the slack (one random instance)."""
    S, R, C = case["x"].shape
    err = np.abs(groupnorm_model(case["x"], case["gamma"], case["beta"], silu).astype(F64) - ref["y"])
    worst = err.reshape(S, R, 32, C // 32).max(axis=(1, 3), keepdims=True)
    return np.broadcast_to(worst, (S, R, 32, C // 32)).reshape(S, R, C)


# C: one vector, 8 lanes partly idle, ragged last vector group (200, 328, 1288), the exact five-vector kernels (320, 640, 2560)
# and the limit 4096; M: one row and the rows-per-block boundary
LN_WIDTHS = (8, 64, 200, 320, 328, 640, 1288, 2560, 4096)
LN_ROWS = (1, 31, 32, 33)


@lru_cache(maxsize=None)
def case_layernorm(M, C):
    """dict(x [M, C], gamma, beta, addvec [ceil(M / rpv), C], rpv, add [M, C] = addvec expanded per row)."""
    rng = np.random.default_rng([M, C, 7])
    x, gamma, beta = _randn16(rng, M, C), _randn16(rng, C), _randn16(rng, C)
    rpv = 8 if M % 8 == 0 else 1
    addvec = _randn16(rng, M // rpv, C)
    add = np.repeat(addvec, rpv, axis=0)
    for a in (x, gamma, beta, addvec, add):
        a.setflags(write=False)
    return dict(x=x, gamma=gamma, beta=beta, addvec=addvec, rpv=rpv, add=add)


LN_SPECIAL_ROWS = ("constant", "constant_negative", "mean_1000_std_1", "outlier_65504", "randn")


@lru_cache(maxsize=None)
def case_layernorm_special(C):
    """One row each of LN_SPECIAL_ROWS: a constant row (-> exactly fp16(beta)), mean 1000 / std 1, one 65504 among randn."""
    rng = np.random.default_rng([C, 11])
    gamma, beta = _randn16(rng, C), _randn16(rng, C)
    x = _randn16(rng, len(LN_SPECIAL_ROWS), C)
    x[0] = 3.140625
    x[1] = -0.0999755859375
    x[2] = f16(1000.0 + x[2])
    x[3, C // 2] = F16_MAX
    for a in (x, gamma, beta):
        a.setflags(write=False)
    return dict(x=x, gamma=gamma, beta=beta)


# N: one element, the scalar tail alone (7), one vector, vector + tail, one stride (2048 = 256 threads x 8) and around it,
# several strides with a tail (2059), the VAE's attention width (9216)
SOFTMAX_WIDTHS = (1, 7, 8, 9, 200, 2047, 2048, 2049, 2059, 9216)
SOFTMAX_SCALES = (1.0, 0.5)
SOFTMAX_ROWS = ("randn_x4", "all_equal", "one_hot")
SOFTMAX_SENTINEL = -7.0


def softmax_ld(N):
    return 8 * ((N + 7) // 8) + 8


@lru_cache(maxsize=None)
def case_softmax(N):
    """x [3, N]: randn * 4, an all-equal row and a one-hot row (65504 against -65504: exactly 1 and 0)."""
    rng = np.random.default_rng([N, 13])
    x = _randn16(rng, 3, N, scale=4.0)
    x[1] = 2.5
    x[2] = -F16_MAX
    x[2, (5 * N) // 7] = F16_MAX
    x.setflags(write=False)
    return x
