"""Exact designs, float64 references, derived slacks, fp32 / fp16 restatements and shared cases for the two fused attention kernels
of csrc/attn.hip (k_attn_spatial, k_attn_temporal; head dimension 64, scale 1/8, no mask).

Plain NumPy, no device code: tests/test_attention_cpu.py shows on the CPU that every check is met by a restatement of the kernel
and that subtly wrong kernels (the `mutant=` arguments) fail one; tests/test_attention_gpu.py feeds the same cases to the HIP
kernels.  The comparison is `check16` of tests/unet_elementwise_ref.py: per element, half an fp16 ulp of the result + a slack that
bounds what the arithmetic may lose before the result is rounded.  No slack is fitted to what a kernel returns.

EXACT DESIGNS.  Logits of exactly 0 for the wanted keys and <= -128 for the rest: exp2 (after the prescale: -184.66 in log2 units)
and __expf flush these to exactly 0 in fp32, so every probability is exactly 1 or 0 and every sum is a sum of integers.
  selection: out[i] == V[pi(i)] bit for bit, any fp16 V;
  subset means: out[i] == mean of integer V rows over subset (i % 64), slack 2^-22 |ref| (one reciprocal, one product, the double
  rounding).
A first tile without a wanted key sets the reference to -184.66; the first wanted key then exceeds it by more than kLazy and the
move rescales the running sums by exp2(-184.66) == 0: the reference-move path is reached with exact arithmetic.

NUMERICAL CASES.  Two float64 references: (a) softmax(q k^T / 8) v on the fp16 inputs; (b) the same with the kernel's documented
operand (spatial: q~ = fp16(fp32(q) c), c = fp32(0.125f * log2(e)f), logits in log2 units; temporal: q~ = fp16(q / 8), exact
unless it goes subnormal).  The slacks are `spatial_slack` and `temporal_slack` below.

Layouts.  A "block" is one (sequence, head) [S, 64] or one (batch, pixel, head) [F, 64]; `spatial_pack` / `temporal_pack` place
blocks [n, L, 64] into the kernels' row-major [rows, heads * 64] matrices (temporal row order (b F + f) HW + pix).
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

from unet_elementwise_ref import ulp16, tol16, worst16, check16, f16, old_close  # noqa: F401  (re-exported to the two test files)

F32, F64, H = np.float32, np.float64, np.float16
A = B = 32.0
LOG2E = math.log2(math.e)
LN2 = math.log(2.0)
C_PRESCALE = F32(0.125) * F32(1.4426950408889634)     # the fp32 product 0.125f * kLog2e of k_attn_spatial
K_LAZY = 8.0                                           # kLazy
NEG_BIG = F32(-1.0e30)                                 # kNegBig
BQ, BKV = 128, 64


# ------------------------------------------------------------------------------------------------ layouts
def spatial_pack(blocks, nseq, S, heads):
    """[nseq * heads, S, 64] (sequence-major) -> [nseq * S, heads * 64]."""
    b = np.asarray(blocks)
    return np.ascontiguousarray(b.reshape(nseq, heads, S, 64).transpose(0, 2, 1, 3).reshape(nseq * S, heads * 64))


def spatial_unpack(a, nseq, S, heads):
    a = np.asarray(a)
    return np.ascontiguousarray(a.reshape(nseq, S, heads, 64).transpose(0, 2, 1, 3).reshape(nseq * heads, S, 64))


def temporal_pack(blocks, Bn, F, HW, heads):
    """[Bn * HW * heads, F, 64] (item = (b HW + pix) heads + head, the kernel's order) -> [Bn * F * HW, heads * 64]."""
    b = np.asarray(blocks)
    return np.ascontiguousarray(b.reshape(Bn, HW, heads, F, 64).transpose(0, 3, 1, 2, 4).reshape(Bn * F * HW, heads * 64))


def temporal_unpack(a, Bn, F, HW, heads):
    a = np.asarray(a)
    return np.ascontiguousarray(a.reshape(Bn, F, HW, heads, 64).transpose(0, 2, 3, 1, 4).reshape(Bn * HW * heads, F, 64))


# ------------------------------------------------------------------------------------------------ exact designs
PIS = ("identity", "random", "reversal", "last", "first")


def make_pi(name, S, n, seed):
    """pi of block n: the named map, shifted by n so that no two blocks of a case share it (n = 0: the map as named)."""
    i = np.arange(S)
    if name == "identity":
        return (i + n) % S
    if name == "reversal":
        return (S - 1 - i + n) % S
    if name == "random":
        return np.random.default_rng([S, n, seed, 1]).permutation(S)
    if name == "last":
        return np.full(S, (S - 1 - n) % S)
    if name == "first":
        return np.full(S, n % S)
    raise ValueError(name)


def selection_block(S, pi, rng):
    """(q, k, v, want) [S, 64] fp16: key pi(i) has logit 0 for query i, every other key -128 or -256 (natural units)."""
    assert 1 <= S <= 1024
    j = np.arange(S)
    k = np.full((S, 64), -B, H)
    k[j, j % 32] = 0.0
    k[j, 32 + j // 32] = 0.0
    q = np.zeros((S, 64), H)
    q[j, pi % 32] = A
    q[j, 32 + pi // 32] = A
    v = (10.0 * rng.standard_normal((S, 64))).astype(H)
    return q, k, v, v[pi].copy()


SUBSET_NAMES = ("all", "last_only", "first_only", "all_but_last", "last_tile", "first_tile", "mod64_63", "even")


def make_subsets(S, n, seed):
    """bool [64, S]: subset a is the set of keys query i with i % 64 == (a - n) % 64 averages over (rotated by the block index n, so
    that short sequences, whose queries reach only the first S dimensions, still meet every named subset in some block).
    Rows 0..7 before the rotation are SUBSET_NAMES; the rest are random with density 0.3.  Every subset is non-empty."""
    rng = np.random.default_rng([S, n, seed, 2])
    j = np.arange(S)
    m = rng.random((64, S)) < 0.3
    m[0] = True
    m[1] = j == S - 1
    m[2] = j == 0
    m[3] = j < S - 1 if S > 1 else True
    m[4] = j >= BKV * ((S - 1) // BKV)
    m[5] = j < BKV
    if S >= 64:
        m[6] = j % 64 == 63
    m[7] = j % 2 == 0
    for a in np.flatnonzero(~m.any(axis=1)):
        m[a, rng.integers(S)] = True
    return np.roll(m, n, axis=0)


def subset_block(S, subsets, rng):
    """(q, k, v, want) with want float64: query i is A e_a, a = i % 64; k[j, a] = -B iff j is not in subset a; V integers in
    [-8, 8] (sums exact in fp32 up to S = 9216: 8 * 9216 < 2^24)."""
    i = np.arange(S)
    q = np.zeros((S, 64), H)
    q[i, i % 64] = A
    k = np.where(subsets.T, 0.0, -B).astype(H)                       # [S, 64]
    v = rng.integers(-8, 9, (S, 64)).astype(H)
    means = (subsets.astype(F64) @ v.astype(F64)) / subsets.sum(axis=1, keepdims=True)      # [64 subsets, 64 d]
    return q, k, v, means[i % 64]


def subset_slack(want):
    return 2.0 ** -22 * np.abs(want)


def _freeze(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _stack(blocks):
    return [np.stack([b[i] for b in blocks]) for i in range(4)]


@lru_cache(maxsize=None)
def case_selection(nseq, S, heads, pi, seed=0):
    """dict(q, k, v [nseq * S, heads * 64] fp16, want the same shape fp16): every (sequence, head) has its own pi and V."""
    blocks = [selection_block(S, make_pi(pi, S, n, seed), np.random.default_rng([S, n, seed, 3])) for n in range(nseq * heads)]
    q, k, v, w = (spatial_pack(a, nseq, S, heads) for a in _stack(blocks))
    return _freeze(dict(q=q, k=k, v=v, want=w))


@lru_cache(maxsize=None)
def case_subsets(nseq, S, heads, seed=0):
    """dict(q, k, v fp16, want float64, sizes [nseq * heads, 64] = the subset sizes)."""
    subs = [make_subsets(S, n, seed) for n in range(nseq * heads)]
    blocks = [subset_block(S, subs[n], np.random.default_rng([S, n, seed, 4])) for n in range(nseq * heads)]
    q, k, v, w = (spatial_pack(a, nseq, S, heads) for a in _stack(blocks))
    return _freeze(dict(q=q, k=k, v=v, want=w, sizes=np.stack([s.sum(axis=1) for s in subs])))


@lru_cache(maxsize=None)
def case_selection_temporal(Bn, F, HW, heads, pi, seed=0):
    n_items = Bn * HW * heads
    blocks = [selection_block(F, make_pi(pi, F, n, seed), np.random.default_rng([F, n, seed, 5])) for n in range(n_items)]
    q, k, v, w = (temporal_pack(a, Bn, F, HW, heads) for a in _stack(blocks))
    return _freeze(dict(q=q, k=k, v=v, want=w))


@lru_cache(maxsize=None)
def case_subsets_temporal(Bn, F, HW, heads, seed=0):
    n_items = Bn * HW * heads
    subs = [make_subsets(F, n, seed) for n in range(n_items)]
    blocks = [subset_block(F, subs[n], np.random.default_rng([F, n, seed, 6])) for n in range(n_items)]
    q, k, v, w = (temporal_pack(a, Bn, F, HW, heads) for a in _stack(blocks))
    return _freeze(dict(q=q, k=k, v=v, want=w, sizes=np.stack([s.sum(axis=1) for s in subs])))


# ------------------------------------------------------------------------------------------------ the cases both files run
# Spatial lengths: 128-query blocks, 64-key tiles, two LDS buffers, 32-query wavefronts, 16-lane query groups.  The (nseq, heads)
# of a length is chosen so that the grid sizes nseq * heads * ceil(S / 128) cover every remainder modulo 8 (xcd_remap).
SPATIAL_SHAPES = {1: (1, 1), 2: (2, 3), 15: (3, 5), 16: (1, 1), 17: (2, 3), 31: (3, 5), 32: (1, 1), 33: (2, 3), 63: (3, 5),
                  64: (1, 1), 65: (2, 3), 127: (3, 5), 128: (1, 1), 129: (2, 3), 191: (3, 5), 192: (1, 1), 193: (2, 3),
                  257: (1, 1), 700: (3, 5), 1024: (2, 3)}
SELECTION_LENGTHS = tuple(SPATIAL_SHAPES)
SELECTION_ALL_PI_AT = (1, 65, 129, 1024)
# subset means: the same lengths, 5 / 7 / 9 blocks exactly, and the benchmark's length (one sequence, one head)
SUBSET_SHAPES = {**SPATIAL_SHAPES, 600: (1, 1), 800: (1, 1), 1100: (1, 1), 9216: (1, 1)}
NUMERICAL_LENGTHS = (45, 130, 700, 1153)
NUMERICAL_KINDS = ("randn", "peaked_3_2", "peaked_5_2", "peaked_4_2", "growth_0.5", "growth_3", "growth_12", "late_dominant",
                   "first_tile_low")
PEAKED_KINDS = ("peaked_3_2", "peaked_5_2", "peaked_4_2")
# (B, F, HW, heads): B HW heads is never a multiple of 4 (the last block has wavefronts without an item)
TEMPORAL_SHAPES = ((1, 1, 1, 1), (1, 2, 33, 1), (2, 7, 1, 5), (1, 14, 33, 5), (3, 16, 1, 1), (1, 17, 33, 1), (1, 25, 1, 5),
                   (2, 31, 33, 1), (1, 32, 33, 5))
TEMPORAL_KINDS = ("randn", "peaked_4_2")


def selection_pis(S):
    return PIS if S in SELECTION_ALL_PI_AT else PIS[:2]


def spatial_blocks(nseq, S, heads):
    return nseq * heads * ((S + BQ - 1) // BQ)


def _randn16(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(H)


@lru_cache(maxsize=None)
def case_numerical(kind, S, seed=0):
    """dict(q, k, v [S, 64] fp16) of one sequence and one head."""
    rng = np.random.default_rng([S, NUMERICAL_KINDS.index(kind), seed, 7])
    q, k, v = _randn16(rng, S, 64), _randn16(rng, S, 64), _randn16(rng, S, 64)
    if kind.startswith("peaked"):
        a, b = (float(x) for x in kind.split("_")[1:])
        q, k = (q.astype(F64) * a).astype(H), (k.astype(F64) * b).astype(H)
    elif kind.startswith("growth"):
        # test_attention_spatial_moving_reference: every query has a positive component along d, the keys' component grows along
        # the sequence from -8 growth to +8 growth
        growth = float(kind.split("_")[1])
        q64 = q.astype(F64)
        d = q64.mean(axis=0)
        d /= np.linalg.norm(d)
        q = (q64 + 2.0 * d).astype(H)
        ramp = np.linspace(-growth * 8.0, growth * 8.0, S)[:, None]
        k = (k.astype(F64) + ramp * d).astype(H)
    elif kind == "late_dominant":
        # test_attention_spatial_peaked_softmax: key 25 S / 32 is aligned with query 7, six times as long
        k[(25 * S) // 32] = (q[7].astype(F64) * 6.0).astype(H)
    elif kind == "first_tile_low":
        q[:, 0] = 8.0
        k[:BKV, 0] = -128.0                                          # -128 + N(0, 63 / 64) in natural units
        assert ((q.astype(F64) @ k.astype(F64)[:BKV].T) / 8.0).max() < -100.0
    return _freeze(dict(q=q, k=k, v=v))


@lru_cache(maxsize=None)
def case_numerical_temporal(kind, Bn, F, HW, heads, seed=0):
    rng = np.random.default_rng([Bn, F, HW, heads, TEMPORAL_KINDS.index(kind), seed, 8])
    rows = Bn * F * HW
    q, k, v = _randn16(rng, rows, 64 * heads), _randn16(rng, rows, 64 * heads), _randn16(rng, rows, 64 * heads)
    if kind == "peaked_4_2":
        q, k = (q.astype(F64) * 4.0).astype(H), (k.astype(F64) * 2.0).astype(H)
    return _freeze(dict(q=q, k=k, v=v))


# ------------------------------------------------------------------------------------------------ float64 references and slacks
def _softmax2(t):
    """Base-2 softmax over the last axis.  Returns (w, R = row maximum, Z = sum 2^(t - R))."""
    R = t.max(axis=-1, keepdims=True)
    e = np.exp2(t - R)
    Z = e.sum(axis=-1, keepdims=True)
    return e / Z, R, Z


def _spread(E, v, o):
    """sum_j E[i, j] |v[j, d] - o[i, d]| for [..., L, L] E, [..., L, 64] v and o (one d at a time: no [L, L, 64] array)."""
    out = np.empty_like(o)
    for d in range(v.shape[-1]):
        out[..., d] = (E * np.abs(v[..., None, :, d] - o[..., :, None, d])).sum(axis=-1)
    return out


def _weights_to_output(E, v, o):
    """Weights that err by at most E_j (absolute, in units of the normalised weights), in the numerator and in the normaliser alike,
    move the output by at most sum_j E_j |v_jd - o_d| / (1 - sum_j E_j): with w~_j = w_j + e_j and sum_j w_j = 1,
        o~ - o = sum_j (w_j + e_j) (v_j - o) / (1 + sum_j e_j) = sum_j e_j (v_j - o) / (1 + sum_j e_j)     exactly.
    The first-order part carries the factor 1, not the 2 of a numerator and a normaliser bounded separately: with 2 a P tile
    rounded to 8 mantissa bits (mutant M5) passes every spatial case."""
    tot = E.sum(axis=-1, keepdims=True)
    assert float(tot.max()) < 0.25, "weight perturbation too large for the bound"
    return _spread(E, v, o) / (1.0 - tot)


def spatial_refs(q, k, v):
    """q, k, v [S, 64] fp16.  dict(ref_a, ref_b, slack_a, slack_b) float64 [S, 64] (see `spatial_slack`)."""
    q64, k64, v64 = (np.asarray(x).astype(F64) for x in (q, k, v))
    c = float(C_PRESCALE)
    qt = (np.asarray(q).astype(F32) * C_PRESCALE).astype(H).astype(F64)
    ta = (q64 @ k64.T) * (LOG2E / 8.0)
    tb = qt @ k64.T
    wa, _, _ = _softmax2(ta)
    wb, Rb, Zb = _softmax2(tb)
    oa, ob = wa @ v64, wb @ v64
    slack_b = spatial_slack(tb, wb, Zb, np.abs(qt) @ np.abs(k64).T, v64, ob)
    # (a): the logits of (b) differ from those of (a) by the rounding of q c to fp16 - (2^-11 + 2^-23) |q_d c| (the fp32 product,
    # then fp16; 2^-25 where the result is subnormal) times |k_jd| - and by c's own rounding, 2^-23 |t| (kLog2e, then the product)
    dq = (2.0 ** -11 + 2.0 ** -23) * np.abs(q64 * c) + 2.0 ** -25
    dlogit = dq @ np.abs(k64).T + 2.0 ** -23 * np.abs(ta)
    slack_a = slack_b + _weights_to_output(wa * np.expm1(LN2 * dlogit), v64, oa)
    return dict(ref_a=oa, ref_b=ob, slack_a=slack_a, slack_b=slack_b)


def spatial_slack(t, w, Z, absprod, v, o):
    """What k_attn_spatial may lose against reference (b), before the final rounding to fp16.  t [S, S]: exact logits in log2 units,
    w their softmax, Z = sum_j 2^(t_j - max t), absprod = sum_d |q~_d k_jd|, v [S, 64], o = w v.

    Score of key j (fp32, log2 units).  Two MFMA k-steps, the first with C = -m, each counted as ONE rounding of 2^-23 relative to
    the magnitude it sums (twice the round-to-nearest unit: no rounding mode of the pipe is assumed), one fp32 subtraction when the
    reference moves, and the rewritten C tuple (-m is rounded once per move, at most once per tile, so old and new probabilities
    disagree about the reference by 2^-24 |m| per move).  |m| <= M = max_j |t_j|, since m is always a tile maximum:
        dscore_j <= 5 * 2^-24 (M + absprod_j) + ntiles 2^-24 M
    Probability: exp2 turns dscore into the relative error expm1(ln 2 dscore); v_exp_f32 adds 2^-22 (one ulp, rounded up); the
    rounding of P to fp16 adds 2^-11 relative where P is normal and 2^-25 absolute where it is subnormal.  P = 2^(t_j - m) with
    m <= max t (the reference never passes the running maximum), so in units of the normalised weights the absolute part is at most
    2^-25 / Z at the least favourable reference m = max t:
        E_j = w_j (expm1(ln 2 dscore_j) + 2^-22) + max(2^-11 w_j, 2^-25 / Z)
    The normaliser sums the SAME rounded P (the ones tile), so `_weights_to_output` applies as it stands.
    P.V chain and normaliser chain (fp32): one step per 32-key MFMA and one product per move, 2^-23 each, of sum_j w_j |v_jd| and
    of 1 (times |o_d|); the reciprocal and the final product add 2^-22 |o_d|."""
    S = t.shape[-1]
    ntiles, nsteps = -(-S // BKV), -(-S // 32)
    M = np.abs(t).max(axis=-1, keepdims=True)
    dscore = 5.0 * 2.0 ** -24 * (M + absprod) + ntiles * 2.0 ** -24 * M
    E = w * (np.expm1(LN2 * dscore) + 2.0 ** -22) + np.maximum(2.0 ** -11 * w, 2.0 ** -25 / Z)
    chain = (nsteps + ntiles) * 2.0 ** -23 * (w @ np.abs(v) + np.abs(o)) + 2.0 ** -22 * np.abs(o)
    return _weights_to_output(E, v, o) + chain


def temporal_refs(q, k, v):
    """q, k, v [n, F, 64] fp16 blocks.  dict(ref_a, ref_b, slack_a, slack_b) float64 [n, F, 64].

    k_attn_temporal against (b) (natural units): four MFMA k-steps of 2^-23 absprod each; the subtraction of the maximum
    (2^-24 (|s| + |max|) <= 2^-23 M); __expf = exp2(x log2(e)): the product's rounding 2^-24 |x| <= 2^-23 M, v_exp_f32 2^-22
    relative:
        dscore_j <= 2^-21 absprod_j + 2^-22 M,   E_j = w_j (expm1(dscore_j) + 2^-22) + eta_j,   eta_j = max(2^-11 w_j, 2^-25 / Z)
    (the maximum IS the reference here, so Z is the plain normaliser).  The row sum is taken over the fp32 e, NOT over the rounded
    P: the fp16 roundings eta_j do not cancel between numerator and normaliser and move the output by up to |o_d| sum_j eta_j on
    top of `_weights_to_output`.  Chains: two P.V MFMA steps (2^-23 sum_j w_j |v_jd| each), 16 additions and one cross-lane
    addition for the sum (17 * 2^-24 |o_d|), the reciprocal and the product (2^-22 |o_d|).
    (a): q / 8 in fp16 is exact unless it is subnormal: 2^-25 sum_d |k_jd| on the logit."""
    q64, k64, v64 = (np.asarray(x).astype(F64) for x in (q, k, v))
    kT = k64.transpose(0, 2, 1)
    qt = (np.asarray(q).astype(H) * H(0.125)).astype(F64)
    ta = (q64 @ kT) * (LOG2E / 8.0)
    tb = (qt @ kT) * LOG2E
    wa, _, _ = _softmax2(ta)
    wb, _, Zb = _softmax2(tb)
    oa, ob = wa @ v64, wb @ v64
    absprod = np.abs(qt) @ np.abs(kT)
    M = np.abs(tb / LOG2E).max(axis=-1, keepdims=True)
    dscore = 2.0 ** -21 * absprod + 2.0 ** -22 * M
    eta = np.maximum(2.0 ** -11 * wb, 2.0 ** -25 / Zb)
    E = wb * (np.expm1(dscore) + 2.0 ** -22) + eta
    tot = E.sum(axis=-1, keepdims=True)
    slack_b = (_weights_to_output(E, v64, ob) + np.abs(ob) * eta.sum(axis=-1, keepdims=True) / (1.0 - tot)
               + 2.0 ** -22 * (wb @ np.abs(v64)) + (17.0 * 2.0 ** -24 + 2.0 ** -22) * np.abs(ob))
    dlogit = 2.0 ** -25 * np.broadcast_to(np.abs(k64).sum(axis=-1)[:, None, :], ta.shape)
    slack_a = slack_b + _weights_to_output(wa * np.expm1(dlogit), v64, oa)
    return dict(ref_a=oa, ref_b=ob, slack_a=slack_a, slack_b=slack_b)


@lru_cache(maxsize=None)
def refs_numerical(kind, S):
    c = case_numerical(kind, S)
    return _freeze(spatial_refs(c["q"], c["k"], c["v"]))


@lru_cache(maxsize=None)
def refs_numerical_temporal(kind, Bn, F, HW, heads):
    """References and slacks in the kernel's packed layout [Bn * F * HW, heads * 64]."""
    c = case_numerical_temporal(kind, Bn, F, HW, heads)
    r = temporal_refs(*(temporal_unpack(c[n], Bn, F, HW, heads) for n in "qkv"))
    return _freeze({n: temporal_pack(a, Bn, F, HW, heads) for n, a in r.items()})


def half_ulps(got, ref):
    """Largest |got - ref| in units of half an fp16 ulp of ref."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return float((np.abs(got - ref) / (0.5 * ulp16(ref))).max())


def old_close_ratio(got, ref, tol=3e-3):
    """Largest |got - ref| as a fraction of what `close()` of tests/test_unet_ops_gpu.py allows (tol * max |ref| + 1e-3)."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    return float(np.abs(got - ref).max() / (tol * (np.abs(ref).max() + 1e-6) + 1e-3))


def median_slack_ratio(slack, ref):
    return float(np.median(np.asarray(slack, F64) / (0.5 * ulp16(ref))))


# ------------------------------------------------------------------------------------------------ restatements
MUTANTS = ("M1", "M2", "M3", "M4", "M5", "M6", "M7", "M8")
M4_DROPPED_KEY = 4999


def _round_mantissa(x, bits):
    """Round fp32 to `bits` explicit mantissa bits (nearest)."""
    m, e = np.frexp(x.astype(F64))
    return np.ldexp(np.round(m * 2.0 ** (bits + 1)) / 2.0 ** (bits + 1), e).astype(F32)


def spatial_model_block(q, k, v, mutant=None):
    """k_attn_spatial for one (sequence, head), q, k, v [S, 64] fp16 -> [S, 64] fp16.  fp16 prescaled Q; per 64-key tile: fp32 scores
    with the reference as the accumulator's start, keys beyond S (which re-read the last row) masked; the reference set by the first
    tile and afterwards moved by max(mx, 0) for ALL 32 queries of a wavefront when any of them exceeds it by more than kLazy, O and
    the row sum rescaled by exp2(-delta); P rounded to fp16; O and the row sum accumulated over the rounded P per 32-key group.
    All wavefronts advance together (the leading axis).
    mutants: M1 V rows r and r + 16 of a 32-key group swapped; M2 the partial tile is not masked; M3 the row sum is not rescaled;
    M4 key M4_DROPPED_KEY is dropped; M5 P rounded to an 8-bit mantissa; M8 every odd tile after the first reuses tile 1."""
    q, k, v = (np.asarray(x) for x in (q, k, v))
    S = q.shape[0]
    qt = (q.astype(F32) * C_PRESCALE).astype(H).astype(F32)
    kf, vf = k.astype(F32), v.astype(F32)
    nw, ntiles = -(-S // 32), -(-S // BKV)
    qi = np.minimum(np.arange(nw * 32), S - 1).reshape(nw, 32)
    Q = qt[qi]                                                         # [nw, 32, 64]
    O = np.zeros((nw, 32, 64), F32)
    L = np.zeros((nw, 32), F32)
    negm = np.zeros((nw, 32), F32)
    swap16 = np.concatenate([np.arange(16, 32), np.arange(16)])
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for t in range(ntiles):
            src = 1 if (mutant == "M8" and t % 2 == 1 and t > 1) else t
            pos = np.arange(t * BKV, (t + 1) * BKV)
            kidx = np.minimum(np.arange(src * BKV, (src + 1) * BKV), S - 1)
            Kt, Vt = kf[kidx], vf[kidx]
            s = negm[:, :, None] + Q[:, :, :32] @ Kt[:, :32].T
            s = s + Q[:, :, 32:] @ Kt[:, 32:].T
            dead = pos >= S
            if mutant == "M2":
                dead = np.zeros_like(dead)
            if mutant == "M4":
                dead = dead | (pos == M4_DROPPED_KEY)
            s[:, :, dead] = NEG_BIG
            mq = s.max(axis=2)
            first = t == 0
            move = np.full(nw, True) if first else (mq > F32(K_LAZY)).any(axis=1)
            delta = np.where(move[:, None], mq if first else np.maximum(mq, F32(0.0)), F32(0.0)).astype(F32)
            if not first:
                alpha = np.exp2(-delta).astype(F32)
                O *= alpha[:, :, None]
                if mutant != "M3":
                    L *= alpha
            s = s - delta[:, :, None]
            negm = negm - delta
            P = np.exp2(s).astype(F32)
            P = _round_mantissa(P, 8) if mutant == "M5" else P.astype(H).astype(F32)
            for G in range(2):
                Pg, Vg = P[:, :, 32 * G:32 * G + 32], Vt[32 * G:32 * G + 32]
                if mutant == "M1":
                    Vg = Vg[swap16]
                L = L + Pg.sum(axis=2, dtype=F32)
                O = O + Pg @ Vg
        out = O * (F32(1.0) / L)[:, :, None]
    return out.reshape(nw * 32, 64)[:S].astype(H)


def spatial_model(q, k, v, nseq, S, heads, mutant=None):
    """The packed form, [nseq * S, heads * 64] -> the same.  M7: the head offset is applied to Q and K but not to V."""
    qb, kb, vb = (spatial_unpack(x, nseq, S, heads) for x in (q, k, v))
    out = []
    for n in range(nseq * heads):
        vn = vb[n - n % heads] if mutant == "M7" else vb[n]
        out.append(spatial_model_block(qb[n], kb[n], vn, None if mutant == "M7" else mutant))
    return spatial_pack(np.stack(out), nseq, S, heads)


def temporal_model_blocks(q, k, v, mutant=None):
    """k_attn_temporal for blocks [n, F, 64] fp16: one 32 x 32 tile; fp16 q / 8; keys >= F (which re-read row F - 1 of K and hold
    zeros in V) masked; exp(s - max); the row sum over the fp32 e; P rounded to fp16.
    mutants: M5 P rounded to an 8-bit mantissa; M6 keys >= F are counted in the row sum."""
    q, k, v = (np.asarray(x) for x in (q, k, v))
    n, F, _ = q.shape
    qt = (q.astype(H) * H(0.125)).astype(F32)
    kidx = np.minimum(np.arange(32), F - 1)
    Kp = k.astype(F32)[:, kidx]                                        # [n, 32, 64]
    Vp = np.zeros((n, 32, 64), F32)
    Vp[:, :F] = v.astype(F32)
    s = np.zeros((n, F, 32), F32)
    for ks in range(4):
        s = s + qt[:, :, 16 * ks:16 * ks + 16] @ Kp[:, :, 16 * ks:16 * ks + 16].transpose(0, 2, 1)
    dead = np.arange(32) >= F
    sm = s.copy()
    sm[:, :, dead] = NEG_BIG
    if mutant == "M6":
        mx = s.max(axis=2, keepdims=True)
        e_sum = np.exp(s - mx).astype(F32)
        e = np.where(dead, F32(0.0), e_sum)
    else:
        mx = sm.max(axis=2, keepdims=True)
        e = e_sum = np.exp(sm - mx).astype(F32)
    ls = e_sum.sum(axis=2, dtype=F32)
    P = _round_mantissa(e, 8) if mutant == "M5" else e.astype(H).astype(F32)
    O = P[:, :, :16] @ Vp[:, :16]
    O = O + P[:, :, 16:] @ Vp[:, 16:]
    return (O * (F32(1.0) / ls)[:, :, None]).astype(H)


def temporal_model(q, k, v, Bn, F, HW, heads, mutant=None):
    """The packed form.  M7: the head offset is applied to Q and K but not to V."""
    qb, kb, vb = (temporal_unpack(x, Bn, F, HW, heads) for x in (q, k, v))
    if mutant == "M7":
        vb = vb[np.arange(vb.shape[0]) // heads * heads]
        mutant = None
    return temporal_pack(temporal_model_blocks(qb, kb, vb, mutant), Bn, F, HW, heads)
