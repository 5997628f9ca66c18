"""float64 / Python-integer reference of the 3DGS-MCMC kernels (csrc/mcmc.hip), written from the formulas of include/syn3r_hip.h:
Philox4x32-10, the Box-Muller normals, Sigma, the gate, the two regularisers, integer sampling with Python ints and the relocation
with `math.comb`.  A helper module of tests/test_mcmc_cpu.py and tests/test_mcmc_gpu.py; numpy only."""
from __future__ import annotations

import bisect
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
TAG_NOISE, TAG_SAMPLE = 0, 1
RATIO_MAX = 51
MASK = 0xFFFFFFFF


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on numpy uint64 arrays holding 32-bit values (or Python ints): -> four arrays of 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in (c0, c1, c2, c3))
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    m32 = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # < 2^64: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m32, p1 >> np.uint64(32), p1 & m32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def words(index, tag: int, step: int, seed: int):
    """The four words of `index` (array or int): counter (index, 0, tag, step), key (seed low, seed high)"""
    seed = int(seed) & (2 ** 64 - 1)
    return philox(index, 0, tag, int(step) & MASK, seed & MASK, seed >> 32)


def normals(index, step: int, seed: int):
    """eps [n,3] float64 and the Box-Muller radius of each component [n,3]"""
    x0, x1, x2, x3 = (w.astype(np.float64) for w in (np.asarray(a) >> np.uint64(8) for a in words(index, TAG_NOISE, step, seed)))
    u0, v1, u2, v3 = (x0 + 1.0) * 2.0 ** -24, x1 * 2.0 ** -24, (x2 + 1.0) * 2.0 ** -24, x3 * 2.0 ** -24
    r01, r2 = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    eps = np.stack([r01 * np.cos(2.0 * np.pi * v1), r01 * np.sin(2.0 * np.pi * v1), r2 * np.cos(2.0 * np.pi * v3)], axis=-1)
    return eps, np.stack([r01, r01, r2], axis=-1)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def gate(o):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-100.0 * (0.005 - np.asarray(o, dtype=np.float64))))


def rotation(q):
    """R [n,3,3] of (w, x, y, z) quaternions [n,4], normalised first"""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def covariance(log_scales, rotations):
    R = rotation(rotations)
    s2 = np.exp(np.asarray(log_scales, dtype=np.float64)) ** 2
    return np.einsum("nik,nk,njk->nij", R, s2, R)


def noise(log_scales, rotations, logits, scale: float, seed: int, step: int, first: int = 0):
    """-> (delta [n,3] = scale gate Sigma eps, magnitude [n,3] = scale gate sum_j |Sigma_ij| (|eps_j| + r_j)) for indices first .."""
    n = len(logits)
    eps, rad = normals(np.arange(first, first + n, dtype=np.uint64), step, seed)
    S = covariance(log_scales, rotations)
    g = float(scale) * gate(sigmoid(logits))
    return g[:, None] * np.einsum("nij,nj->ni", S, eps), g[:, None] * np.einsum("nij,nj->ni", np.abs(S), np.abs(eps) + rad)


def regularisers(logits, log_scales, opacity_reg: float, scale_reg: float):
    """-> (values [2], grad wrt logits [n], grad wrt log-scales [n,3])"""
    o, e = sigmoid(logits), np.exp(np.asarray(log_scales, dtype=np.float64))
    n = o.shape[0]
    return (np.array([opacity_reg * o.mean(), scale_reg * e.mean()]), opacity_reg / n * o * (1.0 - o), scale_reg / (3.0 * n) * e)


def weights(logits_f32, dead_logit_f32):
    """-> (float64 value sigmoid * 65536 before rounding, dead mask); logits and threshold are the fp32 numbers themselves"""
    lg = np.asarray(logits_f32, dtype=np.float32)
    return sigmoid(lg) * 65536.0, lg <= np.float32(dead_logit_f32)


def sample(w, m_extra: int, seed: int, step: int):
    """Integer sampling with Python ints: -> (src [n + m_extra] int64, counts [n] int64)"""
    w = [int(v) for v in w]
    n = len(w)
    excl, total = [], 0
    for v in w:
        excl.append(total)
        total += v
    src = np.full(n + m_extra, -1, dtype=np.int64)
    counts = np.zeros(n, dtype=np.int64)
    if total == 0:
        return src, counts
    dest = [d for d in range(n + m_extra) if d >= n or w[d] == 0]
    if not dest:
        return src, counts
    x0, x1, _, _ = words(np.array(dest, dtype=np.uint64), TAG_SAMPLE, step, seed)
    live = [i for i in range(n) if w[i] > 0]
    keys = [excl[i] for i in live]
    for d, a, b in zip(dest, x0, x1):
        r = (((int(a) << 32) | int(b)) * total) >> 64
        i = live[bisect.bisect_right(keys, r) - 1]
        assert excl[i] <= r < excl[i] + w[i]
        src[d] = i
        counts[i] += 1
    return src, counts


def relocation(o: float, count: int, min_opacity: float):
    """A source of opacity `o` drawn `count` times: -> (new opacity, scale factor o / D, sum |term| / |D|), the double sum as the paper
    writes it, with exact binomials, in float64"""
    ratio = min(count + 1, RATIO_MAX)
    on = -math.expm1(math.log1p(-o) / ratio)
    on = min(max(on, min_opacity), 1.0 - 2.0 ** -23)
    terms = [math.comb(j - 1, k) * (-1.0) ** k * on ** (k + 1) / math.sqrt(k + 1) for j in range(1, ratio + 1) for k in range(j)]
    D = math.fsum(terms)
    return on, o / D, math.fsum(abs(t) for t in terms) / abs(D)
