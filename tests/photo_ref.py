"""Float64 reference, derived slacks, an fp32 restatement with mutants, the designs and the five checks for the fused photometric
loss of csrc/photo_loss.hip (k_photo_fwd, k_photo_bwd, photo_final; with and without a weight map).

NumPy / torch on the CPU, no device code: tests/test_photo_elementwise_cpu.py shows without a GPU that a faithful fp32 restatement of
both kernels meets every check on every design and that subtly wrong kernels (`mutant=`) fail one; tests/test_photo_elementwise_gpu.py
feeds the same designs to the HIP kernels and reads what they leave in the workspace.  No slack is fitted to what a kernel returns.

    L = w [(1 - lam) mean(m |I - G|) + lam mean(m (1 - ssim(I, G)))],   ssim as published: 11-tap Gaussian window, sigma 1.5, zero
    padding, C1 = 0.01^2, C2 = 0.03^2; the window coefficients are the fp32 values make_window() produces, held as float64.

WORKSPACE (photo_workspace_bytes, photo_forward): three maps [3][C][H][W] - d ssim / d mu1 (total), / d sigma1^2, / d sigma12, times
the pixel's weight with a map - then 2 floats per tile (sum |d|, sum ssim), 3 with a map (sum m|d|, sum m ssim, sum m);
tile t = (c gy + tile_y) gx + tile_x.

SLACKS, u = 2^-24, first order.  photo_loss.hip is compiled without contraction: every operation written there rounds once.
  GAMMA = 24: a window moment passes 11 serial FMAs in the horizontal and 11 in the vertical pass, so the product of one tap pair
    meets at most 22 roundings; + 1 for the rounded input product (p p, q q, p q; the means have none) + 1 for the rounded
    coefficient: 22 + 1 + 1.  |moment - exact| <= GAMMA u sum_taps w |term|.
  The element-wise chain from mu1s to d_mu1: every rounded intermediate t contributes |d f / d t| u |t| (2 u |t|, one ulp, for the
    two v_rcp_f32), every moment |d f / d moment| times its bound, C1 and C2 the distance of the kernel's fp32 constants from the
    published ones.  The partials come from float64 autograd with every intermediate a leaf (`_chain`).
  GAMMA_B = 29: k_photo_bwd's window is the same 22 roundings; the combine up (c_l1 s - c_ssim (gx + 2 p gy + q gc)) adds, on the
    longest path (gy): 2p gy, the sum with gx, the sum with q gc, the product with c_ssim, the difference, the product with up: 6;
    + 1 for c_ssim, a double rounded to fp32: 22 + 6 + 1.  The L1 term meets 4: c_l1 rounded, c_l1 (m s), the difference, up.
  DEPTH = 12: block_sum_photo's longest addition chain: 4 serial adds in the thread, 6 butterfly steps in the wave, 2 levels of
    the four-way merge.  A tile sum may err by the sum of its pixels' bounds + DEPTH u sum |v|.

MUTANTS of the restatement (`mutant=`), each one switch:
  M1 the outermost tap dropped in the last column of a tile, horizontal pass of k_photo_fwd;  M2 the same in the last row of
  k_photo_bwd's vertical pass;  M3 replicate padding (the select after the clamped load forgotten);  M4 the halo rows above a last,
  partial tile read one row low;  M5 d_mu1 without its - mu2 d_sg12 term;  M6 the backward's 2 p gA.y written with q;  M7 the
  weight map entering the moments instead of the map value;  M8 a tile remap that collides when nblk % 8 != 0;  M9 the L1 term of
  a partial tile not masked at x >= W or y >= H.  M9 as a mask alone changes nothing - the select has already zeroed those inputs,
  and |0 - 0| adds 0 - so it is the L1 term taken from the loads BEFORE their select, unmasked: the edge pixels are counted again.
"""
from __future__ import annotations

import math
from functools import lru_cache

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
GAMMA = 22 + 1 + 1
GAMMA_B = 22 + 6 + 1
L1_ROUNDINGS = 4
DEPTH = 4 + 6 + 2
KWIN, HALO, TILE, REG, RUN, SPAN, LEAD = 11, 5, 32, 42, 4, 14, 3
ITEMS, THREADS = REG * (TILE // RUN), 256
C1_PUB, C2_PUB = 0.01 ** 2, 0.03 ** 2
C1_F32, C2_F32 = F32(0.01) * F32(0.01), F32(0.03) * F32(0.03)          # the kernel's 0.01f * 0.01f, 0.03f * 0.03f
WEIGHT = 0.7
MUTANTS = ("M1", "M2", "M3", "M4", "M5", "M6", "M7", "M8", "M9")


def window32():
    """make_window(): exp in double, normalised in double, rounded to fp32."""
    g = np.array([math.exp(-float((i - KWIN // 2) ** 2) / (2.0 * 1.5 * 1.5)) for i in range(KWIN)], F64)
    return (g / g.sum()).astype(F32)


def grid(shape):
    C, H, W = shape
    return (H + TILE - 1) // TILE, (W + TILE - 1) // TILE


def coefficients(shape, lam, weight=WEIGHT):
    """(c_l1, c_ssim) as photo_backward forms them: doubles from the float arguments, rounded to fp32."""
    n = float(shape[0]) * shape[1] * shape[2]
    lam, weight = float(F32(lam)), float(F32(weight))
    return F32(weight * (1.0 - lam) / n), F32(weight * lam / n)


# ------------------------------------------------------------------------------------------------ float64 reference
def win64(x):
    """The separable window with zero padding on the last two axes, float64."""
    w = window32().astype(F64)
    x = np.asarray(x, F64)
    H, W = x.shape[-2:]
    xp = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(HALO, HALO), (HALO, HALO)])
    h = sum(w[k] * xp[..., :, k:k + W] for k in range(KWIN))
    return sum(w[k] * h[..., k:k + H, :] for k in range(KWIN))


def _chain(mom, bound):
    """The chain of k_photo_fwd from the five moments to (ssim, d_mu1, d_sg1, d_sg12) in float64 with the published constants, and
    per output the first-order bound of what fp32 may lose.  Each rounded intermediate is `value + delta` with a zero leaf delta:
    d out / d delta is the partial with respect to that intermediate; the function is element-wise, so one backward of out.sum()
    per output gives the per-pixel partials."""
    import torch
    leaves = []

    def leaf(t, err):
        d = torch.zeros_like(t, requires_grad=True)
        leaves.append((d, err))
        return t + d

    def r(t, rel=U):
        return leaf(t, rel * t.detach().abs())

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, F64))
    mu1, mu2, e11, e22, e12 = (leaf(T(m), T(b)) for m, b in zip(mom, bound))
    C1 = leaf(torch.full_like(mu1, C1_PUB), torch.full_like(mu1, abs(float(C1_F32) - C1_PUB)))
    C2 = leaf(torch.full_like(mu1, C2_PUB), torch.full_like(mu1, abs(float(C2_F32) - C2_PUB)))
    mu1s, mu2s, mu12 = r(mu1 * mu1), r(mu2 * mu2), r(mu1 * mu2)
    sg1, sg2, sg12 = r(e11 - mu1s), r(e22 - mu2s), r(e12 - mu12)
    A, B = r(2.0 * mu12 + C1), r(2.0 * sg12 + C2)                       # the products with 2 are exact
    Cc, D = r(r(mu1s + mu2s) + C1), r(r(sg1 + sg2) + C2)
    invC, invD = r(1.0 / Cc, 2.0 * U), r(1.0 / D, 2.0 * U)              # v_rcp_f32: one ulp
    inv = r(invC * invD)
    ssim = r(r(A * B) * inv)
    d_sg1 = r(-ssim * invD)
    d_sg12 = r(2.0 * A * inv)
    t = r(r(r(r(2.0 * mu2 * B) * Cc) - r(r(2.0 * mu1 * A) * B)) * inv)
    d_mu1 = r(r(r(t * invC) - r(2.0 * mu1 * d_sg1)) - r(mu2 * d_sg12))
    outs, bounds = {}, {}
    for name, o in (("ssim", ssim), ("d_mu1", d_mu1), ("d_sg1", d_sg1), ("d_sg12", d_sg12)):
        g = torch.autograd.grad(o.sum(), [d for d, _ in leaves], retain_graph=True, allow_unused=True)
        b = torch.zeros_like(mu1)
        for gi, (_, e) in zip(g, leaves):
            if gi is not None:
                b = b + gi.abs() * e
        outs[name], bounds[name] = o.detach().numpy(), b.numpy()
    return outs, bounds


class Reference:
    """Everything of one (image, target, map) that does not depend on lam, weight or the upstream gradient, in float64."""

    def __init__(self, a, b, m=None):
        self.a32, self.b32 = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
        self.m32 = None if m is None else np.ascontiguousarray(m, F32)
        a, b = self.a32.astype(F64), self.b32.astype(F64)
        self.shape = C, H, W = a.shape
        self.n = C * H * W
        self.m = np.ones((H, W)) if m is None else self.m32.astype(F64)
        self.moments = [win64(a), win64(b), win64(a * a), win64(b * b), win64(a * b)]
        self.moment_bounds = [GAMMA * U * win64(np.abs(t)) for t in (a, b, a * a, b * b, a * b)]
        outs, bounds = _chain(self.moments, self.moment_bounds)
        extra = 0.0 if m is None else U                                  # the product with the weight rounds once more
        self.ssim = self.m * outs["ssim"]
        self.ssim_bound = self.m * bounds["ssim"] + extra * np.abs(self.ssim)
        self.maps = np.stack([self.m * outs[k] for k in ("d_mu1", "d_sg1", "d_sg12")])
        self.map_bounds = np.stack([self.m * bounds[k] for k in ("d_mu1", "d_sg1", "d_sg12")]) + extra * np.abs(self.maps)
        self.l1 = self.m * np.abs(a - b)
        self.l1_bound = (U + extra) * self.l1                            # the difference, the product with the weight
        self.sign = np.sign(a - b)
        gy, gx = grid(self.shape)
        self.tiles = C * gy * gx

        def per_tile(v):
            v = np.broadcast_to(v, (C, H, W))
            p = np.zeros((C, gy * TILE, gx * TILE))
            p[:, :H, :W] = v
            return p.reshape(C, gy, TILE, gx, TILE).sum(axis=(2, 4)).reshape(-1)

        self.count = per_tile(np.ones((C, H, W)))
        self.tile_sums = np.stack([per_tile(self.l1), per_tile(self.ssim), per_tile(self.m)], axis=1)
        self.tile_slack = np.stack([per_tile(self.l1_bound) + DEPTH * U * per_tile(np.abs(self.l1)),
                                    per_tile(self.ssim_bound) + DEPTH * U * per_tile(np.abs(self.ssim)),
                                    DEPTH * U * per_tile(np.abs(self.m))], axis=1)

    # ---- scalars: photo_final sums the tiles in double and rounds each result to fp32 once
    def parts(self, lam, weight=WEIGHT):
        lam, weight = float(F32(lam)), float(F32(weight))
        l1, ss, mm = self.tile_sums.sum(axis=0) / self.n
        s_l1, s_ss, s_mm = self.tile_slack.sum(axis=0) / self.n
        loss = weight * ((1.0 - lam) * l1 + lam * (mm - ss))
        ref = np.array([loss, l1, ss, mm])
        slack = np.array([abs(weight) * ((1.0 - lam) * s_l1 + lam * (s_mm + s_ss)), s_l1, s_ss, s_mm]) + U * np.abs(ref)
        return ref, slack

    # ---- the gradient of up * loss
    def _window_sums(self, maps, bounds=None):
        a, b = self.a32.astype(F64), self.b32.astype(F64)
        w = win64(maps)
        value = w[0] + 2.0 * a * w[1] + b * w[2]
        wa = win64(np.abs(maps))
        S = wa[0] + 2.0 * np.abs(a) * wa[1] + np.abs(b) * wa[2]
        if bounds is None:
            return value, S
        wb = win64(bounds)
        return value, S, wb[0] + 2.0 * np.abs(a) * wb[1] + np.abs(b) * wb[2]

    def grad_autograd(self, lam, up, weight=WEIGHT):
        """float64 autograd of the published loss (conv2d, padding 5, one group per channel), times `up`."""
        import torch
        import torch.nn.functional as Fn
        lam, weight = float(F32(lam)), float(F32(weight))
        C = self.shape[0]
        g = torch.from_numpy(window32().astype(F64))
        win = (g[:, None] @ g[None, :])[None, None].expand(C, 1, KWIN, KWIN).contiguous()
        conv = lambda t: Fn.conv2d(t[None], win, padding=HALO, groups=C)[0]
        x = torch.from_numpy(self.a32.astype(F64)).requires_grad_(True)
        y, m = torch.from_numpy(self.b32.astype(F64)), torch.from_numpy(self.m)
        mu1, mu2 = conv(x), conv(y)
        s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
        ssim = ((2 * mu1 * mu2 + C1_PUB) * (2 * s12 + C2_PUB)) / ((mu1 * mu1 + mu2 * mu2 + C1_PUB) * (s1 + s2 + C2_PUB))
        loss = weight * ((1 - lam) * (m * (x - y).abs()).mean() + lam * (m.expand_as(x) - m * ssim).mean())
        (loss * (1.0 if up is None else up)).backward()
        return x.grad.numpy()

    def grad_end_to_end(self, lam, up, weight=WEIGHT):
        """(float64 autograd gradient, slack): the backward slack + |up c_ssim| times the window sums of the three map bounds."""
        upv = 1.0 if up is None else float(up)
        c_l1, c_ssim = (float(c) for c in coefficients(self.shape, lam, weight))
        _, S, SB = self._window_sums(self.maps, self.map_bounds)
        slack = abs(upv * c_ssim) * (GAMMA_B * U * S + SB) + L1_ROUNDINGS * U * np.abs(upv * c_l1 * self.m * self.sign)
        return self.grad_autograd(lam, up, weight), slack

    def grad_from_stored(self, stored, lam, up, weight=WEIGHT):
        """(the gradient that follows in float64 from the fp32 maps a forward kernel STORED, slack): k_photo_bwd in isolation."""
        upv = 1.0 if up is None else float(up)
        c_l1, c_ssim = (float(c) for c in coefficients(self.shape, lam, weight))
        value, S = self._window_sums(np.asarray(stored, F64))
        l1 = upv * c_l1 * self.m * self.sign
        return l1 - upv * c_ssim * value, abs(upv * c_ssim) * GAMMA_B * U * S + L1_ROUNDINGS * U * np.abs(l1)

    def grad_l1_only_fp32(self, up, weight=WEIGHT):
        """lam = 0: up * (c_l1 * (m * sign)) in fp32, the bits k_photo_bwd must leave (c_ssim is 0)."""
        c_l1, _ = coefficients(self.shape, 0.0, weight)
        s = self.sign.astype(F32) if self.m32 is None else self.m32[None] * self.sign.astype(F32)
        return F32(1.0 if up is None else up) * (c_l1 * s)


# ------------------------------------------------------------------------------------------------ fp32 restatement of the kernels
def fma(a, b, c):
    """v_fma_f32 / v_pk_fma_f32: the exact product (48 bits fit a double) plus the addend, rounded to fp32."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def photo_tile(bid, nblk, mutant=None):
    """photo_tile(): block bid of nblk -> tile index (XCD x takes the x-th contiguous eighth of the tile list)."""
    q, r, xcd, k = nblk // 8, nblk % 8, bid % 8, bid // 8
    if mutant == "M8":
        return xcd * q + k                                               # forgets the r longer eighths: collides when r != 0
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + k


def _load(plane, ys, xs, width, vec, select=True):
    """photo_load20 / photo_load4 for tiles [T]: plane [T, H, W], rows ys [T, R], run starts xs [T, N] -> [T, R, N, width].
    Every load comes from an address clamped into the plane (VEC: a group of four as a whole); the zero is a select afterwards."""
    H, W = plane.shape[-2:]
    rowok = (ys >= 0) & (ys < H)
    yc = np.clip(ys, 0, H - 1)
    if vec:
        g = xs[..., None] + 4 * np.arange(width // 4)                    # [T, N, width / 4]
        cols = (np.clip(g, 0, W - 4)[..., None] + np.arange(4)).reshape(*xs.shape, width)
        ok = np.repeat((g >= 0) & (g < W), 4, axis=-1)
    else:
        e = xs[..., None] + np.arange(width)
        cols, ok = np.clip(e, 0, W - 1), (e >= 0) & (e < W)
    t = np.arange(plane.shape[0])[:, None, None, None]
    v = plane[t, yc[:, :, None, None], cols[:, None]]
    return np.where(rowok[:, :, None, None] & ok[:, None], v, F32(0)) if select else v


def _rows(h, k_drop_last=False):
    """The window over axis -2 of h [..., 42, 32] -> [..., 32, 32], taps in ascending order."""
    w = window32()
    acc = np.zeros(h.shape[:-2] + (TILE, TILE), F32)
    for k in range(KWIN):
        nxt = fma(w[k], h[..., k:k + TILE, :], acc)
        if k_drop_last and k == KWIN - 1:
            nxt[..., TILE - 1, :] = acc[..., TILE - 1, :]
        acc = nxt
    return acc


def _runs(v, k_drop_last=False):
    """The window over the row runs v [..., 42, 8, 14] (inputs kLead .. kLead + 13 of a load) -> [..., 42, 32]."""
    w = window32()
    acc = np.zeros(v.shape[:-1] + (RUN,), F32)
    for k in range(KWIN):
        nxt = fma(w[k], v[..., k:k + RUN], acc)
        if k_drop_last and k == KWIN - 1:
            nxt[..., TILE // RUN - 1, RUN - 1] = acc[..., TILE // RUN - 1, RUN - 1]
        acc = nxt
    return acc.reshape(*acc.shape[:-2], TILE)


def _block_sum(tv):
    """block_sum_photo of per-thread values tv [T, 256]: lane 0's butterfly in each wave, then (r0 + r1) + (r2 + r3)."""
    v = tv.reshape(-1, 4, 64).astype(F32)
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    v = v[..., 0]
    return (v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])


def _serial(terms):
    """0 + t0 + t1 + t2 + t3 over the last axis, in order, fp32."""
    s = np.zeros(terms.shape[:-1], F32)
    for j in range(terms.shape[-1]):
        s = s + terms[..., j]
    return s


def _tiles(shape, mutant):
    """The tiles the grid's blocks work on, in block order: (t, c, y0, x0) arrays."""
    C, H, W = shape
    gy, gx = grid(shape)
    nblk = C * gy * gx
    t = np.array([photo_tile(b, nblk, mutant) for b in range(nblk)])
    c, rem = t // (gy * gx), t % (gy * gx)
    return t, c, (rem // gx) * TILE, (rem % gx) * TILE


def restate_forward(a, b, m=None, vec=None, mutant=None):
    """k_photo_fwd + k_photo_final in fp32: (maps [3, C, H, W], tile sums [tiles, 2 | 3], sums / n [3]), NaN where nothing was
    written.  `vec`: the VEC instantiation (default: W % 4 == 0, as for aligned tensors)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    C, H, W = shape = a.shape
    vec = (W % 4 == 0) if vec is None else vec
    assert not vec or W % 4 == 0
    t, c, y0, x0 = _tiles(shape, mutant)
    T = len(t)
    pa, pb = a[c], b[c]
    ys = y0[:, None] + np.arange(REG) - HALO
    if mutant == "M4":                                                   # halo rows above a last, partial tile: one row low
        low = (y0[:, None] + TILE > H) & (np.arange(REG) < HALO)
        ys = ys - low
    xs = x0[:, None] + np.arange(0, TILE, RUN)
    sel = mutant != "M3"
    p, q = _load(pa, ys, xs - 8, 20, vec, sel)[..., LEAD:LEAD + SPAN], _load(pb, ys, xs - 8, 20, vec, sel)[..., LEAD:LEAD + SPAN]
    if m is not None:
        m = np.ascontiguousarray(m, F32)
        pm = np.broadcast_to(m, (T, H, W))
        mh = _load(pm, ys, xs, RUN, vec)
        if mutant == "M7":                                               # the weight enters the moments ...
            mw = _load(pm, ys, xs - 8, 20, vec)[..., LEAD:LEAD + SPAN]
            p, q = mw * p, mw * q
    drop = mutant == "M1"
    mom = [_rows(_runs(v, drop)) for v in (p, q, p * p, q * q, p * q)]
    # L1 terms of the output rows: item (ry, run) belongs to thread (ry * 8 + run) % 256; no thread owns two output rows
    rowok = (np.arange(REG) >= HALO) & (np.arange(REG) < HALO + TILE) & (ys < H)
    colok = (xs[..., None] + np.arange(RUN)) < W
    pl, ql, okl = p, q, rowok[:, :, None, None] & colok[:, None]
    if mutant == "M9":                                                   # the L1 term reads the loads before their select, unmasked
        pl, ql = (_load(x, ys, xs - 8, 20, vec, False)[..., LEAD:LEAD + SPAN] for x in (pa, pb))
        okl = np.broadcast_to(((np.arange(REG) >= HALO) & (np.arange(REG) < HALO + TILE))[None, :, None, None], okl.shape)
    d = np.abs(pl[..., HALO:HALO + RUN] - ql[..., HALO:HALO + RUN])
    if m is not None:
        d = (_load(pm, ys, xs, RUN, vec, False) if mutant == "M9" else mh) * d
    items = _serial(np.where(okl, d, F32(0))).reshape(T, ITEMS)
    tv = items[:, :THREADS].copy()
    tv[:, :ITEMS - THREADS] += items[:, THREADS:]
    l1_sum = _block_sum(tv)
    # element-wise chain, fp32, one rounding per operation
    mu1, mu2, e11, e22, e12 = mom
    two = F32(2)
    mu1s, mu2s, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sg1, sg2, sg12 = e11 - mu1s, e22 - mu2s, e12 - mu12
    A, B, Cc, D = two * mu12 + C1_F32, two * sg12 + C2_F32, mu1s + mu2s + C1_F32, sg1 + sg2 + C2_F32
    invC, invD = F32(1) / Cc, F32(1) / D
    inv = invC * invD
    ssim = A * B * inv
    d_sg1 = -ssim * invD
    d_sg12 = two * A * inv
    d_mu1 = (two * mu2 * B * Cc - two * mu1 * A * B) * inv * invC - two * mu1 * d_sg1
    if mutant != "M5":
        d_mu1 = d_mu1 - mu2 * d_sg12
    yy, xx = y0[:, None] + np.arange(TILE), x0[:, None] + np.arange(TILE)
    ok = (yy < H)[:, :, None] & (xx < W)[:, None, :]
    if m is not None:
        mv = pm[np.arange(T)[:, None, None], np.minimum(yy, H - 1)[:, :, None], np.minimum(xx, W - 1)[:, None, :]]
        if mutant != "M7":                                               # ... instead of the map value
            d_mu1, d_sg1, d_sg12, ssim = mv * d_mu1, mv * d_sg1, mv * d_sg12, mv * ssim
    maps = np.full((3, C, H, W), np.nan, F32)
    ti, yi, xi = np.nonzero(ok)
    for k, v in enumerate((d_mu1, d_sg1, d_sg12)):
        maps[k, c[ti], yy[ti, yi], xx[ti, xi]] = v[ti, yi, xi]
    thread = lambda v: _serial(np.where(ok, v, F32(0)).reshape(T, TILE // RUN, RUN, TILE).transpose(0, 1, 3, 2)).reshape(T, THREADS)
    sums = [l1_sum, _block_sum(thread(ssim))] + ([_block_sum(thread(mv))] if m is not None else [])
    partial = np.full((T, len(sums)), np.nan, F32)
    partial[t] = np.stack(sums, axis=1)
    return maps, partial


def restate_final(partial, shape, lam, weight=WEIGHT):
    """photo_final: double sums of the tile slots, each result rounded to fp32 once: [loss, L1, SSIM (, mean m)]."""
    n = float(shape[0]) * shape[1] * shape[2]
    lam, weight = float(F32(lam)), float(F32(weight))
    s = partial.astype(F64).sum(axis=0) * (1.0 / n)
    if partial.shape[1] == 3:
        return np.array([weight * ((1.0 - lam) * s[0] + lam * (s[2] - s[1])), s[0], s[1], s[2]]).astype(F32)
    return np.array([weight * ((1.0 - lam) * s[0] + lam * (1.0 - s[1])), s[0], s[1]]).astype(F32)


def restate_backward(a, b, maps, lam, up, m=None, vec=None, weight=WEIGHT, mutant=None):
    """k_photo_bwd in fp32 on the maps a forward left: the image gradient [C, H, W]."""
    a, b, maps = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32), np.ascontiguousarray(maps, F32)
    C, H, W = shape = a.shape
    vec = (W % 4 == 0) if vec is None else vec
    c_l1, c_ssim = coefficients(shape, lam, weight)
    t, c, y0, x0 = _tiles(shape, mutant)
    T = len(t)
    ys = y0[:, None] + np.arange(REG) - HALO
    xs = x0[:, None] + np.arange(0, TILE, RUN)
    g = [_rows(_runs(_load(maps[k][c], ys, xs - 8, 20, vec)[..., LEAD:LEAD + SPAN]), mutant == "M2") for k in range(3)]
    yy, xx = y0[:, None] + np.arange(TILE), x0[:, None] + np.arange(TILE)
    ok = (yy < H)[:, :, None] & (xx < W)[:, None, :]
    at = lambda pl: pl[np.arange(T)[:, None, None], np.minimum(yy, H - 1)[:, :, None], np.minimum(xx, W - 1)[:, None, :]]
    p, q = at(a[c]), at(b[c])
    d = p - q
    sgn = np.where(d > 0, F32(1), np.where(d < 0, F32(-1), F32(0))).astype(F32)
    if m is not None:
        sgn = at(np.broadcast_to(np.ascontiguousarray(m, F32), (T, H, W))) * sgn
    two = F32(2)
    win = g[0] + two * (q if mutant == "M6" else p) * g[1] + q * g[2]
    val = F32(1.0 if up is None else up) * (c_l1 * sgn - c_ssim * win)
    grad = np.full(shape, np.nan, F32)
    ti, yi, xi = np.nonzero(ok)
    grad[c[ti], yy[ti, yi], xx[ti, xi]] = val[ti, yi, xi]
    return grad


# ------------------------------------------------------------------------------------------------ designs
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def make_map(kind, H, W, seed=0):
    """random; a rectangle crossing x = 32 and y = 32 (clipped to the image); random with exact zeros."""
    if kind is None:
        return None
    if kind == "rectangle":
        m = np.zeros((H, W), F32)
        m[7:35, 5:34] = 1.0
        return m
    r = _rng(H, W, seed, 7)
    m = r.random((H, W), dtype=F32)
    if kind == "zeros":
        m[r.random((H, W)) < 0.3] = 0.0
        m[:, W // 2] = 0.0
    return m


def sweep_images(shape, seed=0, ties=False):
    """rand against rand + 0.2 randn, unclamped: some values lie outside [0, 1], as a raw render's do.  `ties`: every seventh target
    value is the image's (sign 0)."""
    r = _rng(*shape, seed, 1)
    a = r.random(shape, dtype=F32)
    b = (a + F32(0.2) * r.standard_normal(shape, dtype=F32)).astype(F32)
    if ties:
        b.reshape(-1)[::7] = a.reshape(-1)[::7]
    return a, b


# (shape, lam, up, map): W % 4 in {0,1,2,3}; W in {1,2,3,4,8,11,12}; H in {1,5,11}; sides 31..33, 63..65; C in {1,3,5};
# tiles C gx gy in {1,2,3,5,6,7,8,9,12,15,16,17,23} (every residue mod 8; q = 0 and q > 0 in photo_tile) and 60
GEOMETRY = [((1, 1, 1), 0.2, 1.5, None), ((1, 5, 2), 0.2, None, "random"), ((3, 11, 3), 1.0, 1.5, None), ((5, 1, 4), 0.2, 1.5, "random"),
            ((1, 5, 8), 0.0, None, None), ((1, 11, 11), 0.2, None, "zeros"), ((1, 31, 12), 0.2, 1.5, None),
            ((1, 32, 33), 0.2, 1.5, "zeros"), ((1, 5, 197), 1.0, None, "random"), ((1, 64, 100), 0.2, 1.5, None),
            ((1, 64, 100), 0.2, None, "rectangle"), ((1, 65, 65), 0.2, 1.5, "rectangle"), ((3, 64, 63), 0.2, 1.5, None),
            ((3, 64, 63), 0.0, 1.5, "random"), ((5, 31, 65), 0.2, None, None), ((1, 100, 128), 0.2, 1.5, "random"),
            ((1, 11, 530), 0.2, 1.5, None), ((1, 5, 735), 0.2, None, "zeros"), ((3, 37, 53), 0.2, 1.5, "random"),
            ((3, 31, 33), 0.2, None, None),            ((3, 97, 131), 0.2, 1.5, None), ((3, 97, 131), 1.0, None, "rectangle")]
ALIGNMENT = [((1, 64, 100), "random"), ((1, 31, 12), "random")]          # W % 4 == 0: also run at a storage offset of one float
# (image, target, map, workspace) offset by one float; the workspace's alignment chooses k_photo_bwd's instantiation
OFFSETS = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (1, 1, 1, 0), (0, 0, 0, 1)]
CONDITIONING_SHAPES = [(1, 37, 44), (1, 37, 45)]                         # VEC and not, 2 x 2 tiles
CONDITIONING = ("flat_1.0", "flat_0.9", "flat_0.5", "const_0.7_0.7", "const_0.7_0.3", "zeros_zeros", "zeros_rand", "anticorrelated",
                "equal_random", "equal_flat_bright", "checkerboard")
EQUAL = ("const_0.7_0.7", "zeros_zeros", "equal_random", "equal_flat_bright")     # image == target


def conditioning_images(name, shape):
    r = _rng(*shape, 3)
    noise = lambda s: (s * (2.0 * r.random(shape) - 1.0))
    one = np.ones(shape)
    if name == "flat_1.0":
        a = 1.0 + noise(1e-3)
        b = a + noise(1e-3)
    elif name == "flat_0.9":
        a, b = 0.9 + noise(3e-3), 0.9 + noise(3e-3)
    elif name == "flat_0.5":
        a, b = 0.5 + noise(1e-3), 0.5 + noise(1e-3)
    elif name == "const_0.7_0.7":
        a, b = 0.7 * one, 0.7 * one
    elif name == "const_0.7_0.3":
        a, b = 0.7 * one, 0.3 * one
    elif name == "zeros_zeros":
        a, b = 0 * one, 0 * one
    elif name == "zeros_rand":
        a, b = 0 * one, r.random(shape)
    elif name == "anticorrelated":
        a = r.random(shape)
        b = 1.0 - a
    elif name == "equal_random":
        a = r.random(shape)
        b = a
    elif name == "equal_flat_bright":
        a = 1.0 + noise(1e-3)
        b = a
    elif name == "checkerboard":
        y, x = np.indices(shape[1:])
        a = np.broadcast_to((((y // 4) + (x // 4)) % 2).astype(F64), shape)
        b = 1.0 - a
    else:
        raise ValueError(name)
    return np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)


class Case:
    def __init__(self, family, name, shape, lam, up, kind, images):
        self.family, self.name, self.shape, self.lam, self.up, self.kind, self._images = family, name, shape, lam, up, kind, images

    def __repr__(self):
        return self.name

    @property
    def data(self):
        """(image, target, map or None) fp32, and the float64 Reference: built once per case."""
        return _case_data(self)


@lru_cache(maxsize=None)
def _case_data(case):
    a, b = case._images()
    m = make_map(case.kind, case.shape[1], case.shape[2])
    return a, b, m, Reference(a, b, m)


def _cases():
    out = []
    for i, (shape, lam, up, kind) in enumerate(GEOMETRY):
        out.append(Case("geometry", "geom-%dx%dx%d-lam%g-up%s-%s" % (*shape, lam, up, kind), shape, lam, up, kind,
                        lambda shape=shape, i=i, lam=lam: sweep_images(shape, i, ties=lam == 0.0)))      # lam = 0: with exact ties
    for shape, kind in ALIGNMENT:
        out.append(Case("alignment", "align-%dx%dx%d" % shape, shape, 0.2, 1.5, kind, lambda shape=shape: sweep_images(shape, 99)))
    for shape in CONDITIONING_SHAPES:
        for name in CONDITIONING:
            out.append(Case("conditioning", "%s-%dx%dx%d" % (name, *shape), shape, 0.2, 1.5, None,
                            lambda name=name, shape=shape: conditioning_images(name, shape)))
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}

# ---- shift design: a 20 x 24 random patch (image and target) in a zero canvas
PATCH = (20, 24)
CANVASES = [(3, 80, 84), (3, 80, 83)]
SHIFTS = [(o, o) for o in range(37)] + [(0, 60), (56, 0), (60, 59)]
CANONICAL = (10, 10)                                                     # patch and surround well inside both canvases
SURROUND = HALO


@lru_cache(maxsize=None)
def shift_patch():
    r = _rng(20, 24, 5)
    return r.random((3,) + PATCH, dtype=F32), r.random((3,) + PATCH, dtype=F32)


def shift_images(canvas, offset):
    """The patch at `offset` (clipped where the canvas ends), zeros elsewhere."""
    C, H, W = canvas
    pa, pb = shift_patch()
    a, b = np.zeros(canvas, F32), np.zeros(canvas, F32)
    oy, ox = offset
    h, w = min(PATCH[0], H - oy), min(PATCH[1], W - ox)
    a[:, oy:oy + h, ox:ox + w], b[:, oy:oy + h, ox:ox + w] = pa[:, :h, :w], pb[:, :h, :w]
    return a, b


def _dilate(mask, r):
    p = np.pad(mask, r)
    H, W = mask.shape
    out = np.zeros_like(mask)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def shift_region(canvas, offset):
    """The patch with its 5-pixel surround, in patch coordinates ([-5, 25) x [-5, 29)) -> (canvas index arrays ys, xs of the part
    inside the canvas, region index arrays ry, rx, masks of that part where the maps resp. the gradient must be bit-identical to
    every other offset's).  'Wherever the canvas contains them', made exact: a stored map value depends on the patch pixels within
    5 of it, so it is comparable when none of those fell off the canvas; a gradient value depends on the map values within 5 of it
    that are not the far field's - those of the region - so it is comparable when all of them are inside the canvas and comparable
    themselves.  (Outside the patch image and target are 0, so only d_mu1 enters, and d_mu1 is exactly 0 outside the region.)"""
    _, H, W = canvas
    oy, ox = offset
    s = SURROUND
    ry, rx = np.arange(-s, PATCH[0] + s), np.arange(-s, PATCH[1] + s)
    inside = ((ry + oy >= 0) & (ry + oy < H))[:, None] & ((rx + ox >= 0) & (rx + ox < W))[None, :]
    patch = ((ry >= 0) & (ry < PATCH[0]))[:, None] & ((rx >= 0) & (rx < PATCH[1]))[None, :]
    maps_bad = _dilate(patch & ~inside, HALO)
    grad_bad = _dilate(~inside | maps_bad, HALO)
    return inside, ry + oy, rx + ox, inside & ~maps_bad, inside & ~grad_bad


def far_field(canvas, offset):
    """bool [H, W]: pixels whose window does not reach the patch - all five moments are exactly 0 there."""
    _, H, W = canvas
    near = np.zeros((H, W), bool)
    oy, ox = offset
    near[max(oy - HALO, 0):oy + PATCH[0] + HALO, max(ox - HALO, 0):ox + PATCH[1] + HALO] = True
    return ~near


def far_d_sg1():
    """-1 * rcp(C2) in fp32: d_sg1 where the SSIM map value is 1."""
    return -(F32(1) / C2_F32)


def ulps(x, y):
    """|x - y| in units of the fp32 spacing at y."""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    return np.abs(x.astype(F64) - y.astype(F64)) / np.spacing(np.abs(y)).astype(F64)


# ------------------------------------------------------------------------------------------------ the checks
class CheckFailed(AssertionError):
    def __init__(self, check, msg, worst=float("inf")):
        super().__init__("check %s: %s" % (check, msg))
        self.check, self.worst = check, worst


def _worst(check, what, got, ref, slack):
    """max err / slack over every element; nothing is skipped: a bound that is not finite, a value that is not, or an error above
    its bound fails.  err == 0 counts as 0 also where the slack is 0."""
    got, ref, slack = np.asarray(got, F64), np.asarray(ref, F64), np.asarray(slack, F64)
    if not np.isfinite(slack).all() or not np.isfinite(ref).all():
        raise CheckFailed(check, "%s: the reference or its bound is not finite" % what)
    if not np.isfinite(got).all():
        raise CheckFailed(check, "%s: %d values are not finite (never written, or NaN)" % (what, int((~np.isfinite(got)).sum())))
    err = np.abs(got - ref)
    ratio = np.where(err == 0, 0.0, err / np.where(slack > 0, slack, 1.0))
    ratio = np.where((err > 0) & (slack <= 0), np.inf, ratio)
    w = float(ratio.max()) if ratio.size else 0.0
    if not w <= 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise CheckFailed(check, "%s: err / tol %.3g at %s (got %.9g, reference %.9g, tol %.3g)"
                          % (what, w, i, got[i], ref[i], slack[i]), w)
    return w


def check_forward_pixels(ref, maps):
    """Check 1: each stored map within its derived bound of the float64 map, every in-image element written."""
    return max(_worst(1, name, maps[k], ref.maps[k], ref.map_bounds[k]) for k, name in enumerate(("d_mu1", "d_sg1", "d_sg12")))


def check_forward_tiles(ref, partial, parts, lam, equal=False, weight=WEIGHT):
    """Check 2: every tile slot within the tile slack of the float64 sums of THAT tile; the scalars within the slack of summing
    the tiles in double.  `equal` (image == target, no map): L1 exactly 0, tile SSIM sums within count * 4u of the pixel count,
    parts[2] within 4u of 1."""
    per = partial.shape[1]
    if partial.shape[0] != ref.tiles or per != (2 if ref.m32 is None else 3):
        raise CheckFailed(2, "tile slots %s for %d tiles" % (partial.shape, ref.tiles))
    w = max(_worst(2, name, partial[:, k], ref.tile_sums[:, k], ref.tile_slack[:, k])
            for k, name in list(enumerate(("tile sum |d|", "tile sum ssim", "tile sum m")))[:per])
    pref, pslack = ref.parts(lam, weight)
    w = max(w, _worst(2, "parts", parts, pref[:len(parts)], pslack[:len(parts)]))
    if equal:
        if not (np.all(partial[:, 0] == 0) and parts[1] == 0):
            raise CheckFailed(2, "image == target: the L1 part is not exactly 0")
        _worst(2, "tile sum ssim against the pixel count", partial[:, 1], ref.count, ref.count * 4 * U)
        _worst(2, "parts[2] against 1", parts[2], 1.0, 4 * U)
    return w


def check_backward_isolated(ref, stored, grad, lam, up, weight=WEIGHT):
    """Check 3: the gradient within the backward slack of the float64 window sums of the maps the forward STORED; lam = 0: the
    bits of up * (c_l1 * (m * sign)), zeros at ties."""
    g, slack = ref.grad_from_stored(stored, lam, up, weight)
    w = _worst(3, "gradient from the stored maps", grad, g, slack)
    if float(F32(lam)) == 0.0 and not np.array_equal(np.asarray(grad, F32), ref.grad_l1_only_fp32(up, weight)):
        raise CheckFailed(3, "lam = 0: the gradient is not up * (c_l1 * sign) bit for bit")
    return w


def check_end_to_end(ref, grad, lam, up, weight=WEIGHT):
    """Check 4: the gradient against float64 autograd of the published loss."""
    g, slack = ref.grad_end_to_end(lam, up, weight)
    return _worst(4, "gradient against float64 autograd", grad, g, slack)


def check_bits(what, got, want):
    """Check 5: bit for bit (NaN patterns included)."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    if got.shape != want.shape or not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        n = int((got.view(np.uint32) != want.view(np.uint32)).sum()) if got.shape == want.shape else -1
        raise CheckFailed(5, "%s: %d of %d values differ in their bits" % (what, n, got.size))


def _region_values(canvas, offset, maps, grad):
    _, ys, xs, ok_maps, ok_grad = shift_region(canvas, offset)
    yc, xc = np.clip(ys, 0, canvas[1] - 1), np.clip(xs, 0, canvas[2] - 1)
    return maps[:, :, yc[:, None], xc[None, :]], grad[:, yc[:, None], xc[None, :]], ok_maps, ok_grad


def check_shift(runs):
    """Check 5 on the shift design.  runs: {(canvas, offset): (maps [3,C,H,W], grad [C,H,W])}, CANONICAL among the offsets of each
    canvas.  Over the patch and its surround the maps are bit-identical at every offset and on both canvases, the gradient at every
    offset of one canvas (c_ssim depends on the canvas' size); in the far field d_sg1 is -1 * rcp(C2) within 2 ulp."""
    want_maps, _, ok, _ = _region_values(CANVASES[0], CANONICAL, *runs[(CANVASES[0], CANONICAL)])
    assert ok.all()
    for (canvas, offset), (maps, grad) in runs.items():
        _, want_grad, _, ok = _region_values(canvas, CANONICAL, *runs[(canvas, CANONICAL)])
        assert ok.all()
        rm, rg, ok_maps, ok_grad = _region_values(canvas, offset, maps, grad)
        check_bits("shift maps on %s at %s" % (canvas, offset), np.where(ok_maps, rm, F32(0)), np.where(ok_maps, want_maps, F32(0)))
        check_bits("shift gradient on %s at %s" % (canvas, offset), np.where(ok_grad, rg, F32(0)), np.where(ok_grad, want_grad, F32(0)))
        far = far_field(canvas, offset)
        d = ulps(maps[1][:, far], far_d_sg1())
        if d.size and not d.max() <= 2:
            raise CheckFailed(5, "shift %s at %s: far-field d_sg1 is %.3g ulp from -rcp(C2)" % (canvas, offset, d.max()))


# ------------------------------------------------------------------------------------------------ the criteria the suite had before
def old_criteria_pass(ref, parts, grad, lam, up, weight=WEIGHT):
    """mean SSIM within 2e-5, mean L1 within 2e-6, the gradient within rtol 2e-3, atol 2e-7 + 2e-4 max|grad| of float64 autograd."""
    pref, _ = ref.parts(lam, weight)
    g = ref.grad_autograd(lam, up, weight)
    if not np.isfinite(np.asarray(parts, F64)).all() or not np.isfinite(grad).all():
        return False
    ok_g = np.all(np.abs(grad - g) <= 2e-7 + 2e-4 * np.abs(g).max() + 2e-3 * np.abs(g))
    return bool(abs(parts[2] - pref[2]) < 2e-5 and abs(parts[1] - pref[1]) < 2e-6 and ok_g)
