"""Float64 restatement of the multi-view photometric reprojection term (include/syn3r_hip.h, csrc/reproj.hip), the cases the CPU
and GPU tests share, the first-order fp32 error model their bounds come from, and the abstract descent design.  Plain torch / numpy on
the CPU; imports nothing from the product's operator.  Every function takes the SAME fp32 inputs the kernel gets and promotes them
to float64.

The error model (U = 2^-24, the unit roundoff of fp32; first order, each factor counts the kernel's operations on the quantity):
    r = (x - c) / f                      2 operations                                |dr|  <= 2 U |r|
    A = (m0 rx + m1 ry) + m2             2 products, 2 sums, on inputs 2 U off       |dA|  <= 6 U (|m0 rx| + |m1 ry| + |m2|)
    X = z A + t      z = D / a (1 op)    1 product, 1 sum                            |dX|  <= |z| |dA| + 3 U (|z A| + |t|)
    q = (f X_x) / X_z + c                product, quotient, sum                      |dq|  <= f (|dX_x| + |X_x / X_z| |dX_z|) / X_z
                                                                                             + 3 U |f X_x / X_z| + U |q|
    I(q) bilinear: 2 differences, 6 products, 3 sums on fractions |dq| off           |dI|  <= 8 U max|tap| + |I_x| |dq_x| + |I_y| |dq_y|
    I_x = gy1 (i01 - i00) + fy (i11 - i10)                                           |dI_x| <= |cross| |dq_y| + 6 U sum|tap|
    dq/dz = f (A_x t_z - A_z t_x) / X_z^2                                            |d(dq/dz)| <= f (|dA| (|t_z| + |t_x|) + 3 U (|A_x t_z| + |A_z t_x|)) / X_z^2
                                                                                             + |dq/dz| (2 |dX_z| / X_z + 4 U)
Every margin and bound of the tests is SAFETY = 2 times the first-order figure (the second-order terms)."""
import math
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24
SAFETY = 2.0
ZNEAR = 0.01
F64 = torch.float64


def _f64(t):
    """float64 of what the caller hands over: fp32 tensors and arrays are promoted exactly (float64 ones, of the CPU tests, are kept)"""
    return (t.detach().cpu() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))).to(F64)


def term(depth, alpha, target, sources, views, weight=1.0, alpha_min=0.5, autograd=False):
    """The term in float64.  depth, alpha [H,W] (or [1,H,W]), target [3,H,W], sources: list of [3,H,W], views = (target_k [4],
    table [S,16]), all fp32.  -> namespace: loss, parts [4], e [H,W] (0 where dead), src [H,W] int64 (-1 dead), n_live, dz [H,W] (the
    UNSCALED dL/dz, weight / N_live = 1), g_depth, g_alpha [H,W], and per source lists q (2 x [H,W]), Xz, valid, e_s plus the
    error model's figures (dq, de_s, ...).  `autograd`: also ag_depth, ag_alpha = float64 autograd of a torch restatement of the
    loss, through D / a."""
    D = _f64(depth).reshape(depth.shape[-2:])
    a = _f64(alpha).reshape(D.shape)
    It = _f64(target)
    H, W = D.shape
    tk = _f64(views[0]).reshape(4)
    table = _f64(views[1]).reshape(-1, 16)
    S = table.shape[0]
    amin = float(np.float32(alpha_min))
    w = float(np.float32(weight))
    if autograd:
        D = D.clone().requires_grad_(True)
        a = a.clone().requires_grad_(True)
    live0 = (a.detach() >= amin) & (D.detach() > 0)
    one = torch.ones_like(D.detach())
    z = torch.where(live0, D / torch.where(live0, a, one), one)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    rx, ry = (xs - tk[2]) / tk[0], (ys - tk[3]) / tk[1]
    out = SimpleNamespace(q=[], Xz=[], valid=[], e_s=[], dz_s=[], dq=[], de_s=[], dval=[], diff=[], ddz_s=[], dqz=[], H=H, W=W, S=S)
    zd = z.detach()
    for s in range(S):
        m, t, (fx, fy, cx, cy) = table[s, :9], table[s, 9:12], table[s, 12:16]
        Is = _f64(sources[s])
        A = [m[3 * i] * rx + m[3 * i + 1] * ry + m[3 * i + 2] for i in range(3)]
        X = [z * A[i] + t[i] for i in range(3)]
        Xz = X[2]
        qx, qy = fx * X[0] / Xz + cx, fy * X[1] / Xz + cy
        qxd, qyd, Xzd = qx.detach(), qy.detach(), Xz.detach()
        valid = (Xzd >= ZNEAR) & (qxd >= 0) & (qxd <= W - 1) & (qyd >= 0) & (qyd <= H - 1)
        sx, sy = torch.where(valid, qx, torch.zeros_like(qx)), torch.where(valid, qy, torch.zeros_like(qy))
        x0 = sx.detach().floor().clamp(max=W - 2).long()
        y0 = sy.detach().floor().clamp(max=H - 2).long()
        fxx, fyy = sx - x0, sy - y0
        tap = lambda dy, dx: Is[:, y0 + dy, x0 + dx]
        i00, i01, i10, i11 = tap(0, 0), tap(0, 1), tap(1, 0), tap(1, 1)
        val = (1 - fyy) * ((1 - fxx) * i00 + fxx * i01) + fyy * ((1 - fxx) * i10 + fxx * i11)
        diff = val - It
        e_s = diff.abs().sum(0) / 3.0
        # the analytic gradient, on detached values
        with torch.no_grad():
            fxd, fyd = fxx.detach(), fyy.detach()
            gx = (1 - fyd) * (i01 - i00) + fyd * (i11 - i10)
            gy = (1 - fxd) * (i10 - i00) + fxd * (i11 - i01)
            Ad = [v.detach() for v in A]
            dqx = fx * (Ad[0] * t[2] - Ad[2] * t[0]) / Xzd ** 2
            dqy = fy * (Ad[1] * t[2] - Ad[2] * t[1]) / Xzd ** 2
            sg = torch.sign(diff.detach())
            dz_s = (sg * (gx * dqx + gy * dqy)).sum(0) / 3.0
            # the error model (module docstring)
            absA = [(m[3 * i] * rx).abs() + (m[3 * i + 1] * ry).abs() + m[3 * i + 2].abs() for i in range(3)]
            dA = [6 * U * v for v in absA]
            dX = [zd.abs() * dA[i] + 3 * U * ((zd * Ad[i]).abs() + t[i].abs()) for i in range(3)]
            Xd = [v.detach() for v in X]
            safe = Xzd.abs().clamp(min=1e-30)
            dq_x = fx.abs() * (dX[0] + (Xd[0] / safe).abs() * dX[2]) / safe + 3 * U * (fx * Xd[0] / safe).abs() + U * qxd.abs()
            dq_y = fy.abs() * (dX[1] + (Xd[1] / safe).abs() * dX[2]) / safe + 3 * U * (fy * Xd[1] / safe).abs() + U * qyd.abs()
            tapmax = torch.stack([i00.abs(), i01.abs(), i10.abs(), i11.abs()]).max(0).values
            tapsum = i00.abs() + i01.abs() + i10.abs() + i11.abs()
            dval = 8 * U * tapmax + gx.abs() * dq_x + gy.abs() * dq_y                      # [3,H,W]
            de = (dval + U * It.abs()).sum(0) / 3.0 + 4 * U * e_s.detach()
            cross = (i11 - i10 - i01 + i00).abs()
            dgx, dgy = cross * dq_y + 6 * U * tapsum, cross * dq_x + 6 * U * tapsum
            ddqx = fx.abs() * (dA[0] * t[2].abs() + dA[2] * t[0].abs() + 3 * U * ((Ad[0] * t[2]).abs() + (Ad[2] * t[0]).abs())) / safe ** 2 \
                + dqx.abs() * (2 * dX[2] / safe + 4 * U)
            ddqy = fy.abs() * (dA[1] * t[2].abs() + dA[2] * t[1].abs() + 3 * U * ((Ad[1] * t[2]).abs() + (Ad[2] * t[1]).abs())) / safe ** 2 \
                + dqy.abs() * (2 * dX[2] / safe + 4 * U)
            ddz = (dgx * dqx.abs() + gx.abs() * ddqx + dgy * dqy.abs() + gy.abs() * ddqy).sum(0) / 3.0 \
                + 6 * U * ((gx * dqx).abs() + (gy * dqy).abs()).sum(0) / 3.0
        out.q.append((qxd, qyd)); out.Xz.append(Xzd); out.valid.append(valid); out.e_s.append(e_s); out.dz_s.append(dz_s)
        out.dq.append((dq_x, dq_y)); out.de_s.append(de); out.dval.append(dval); out.diff.append(diff.detach()); out.ddz_s.append(ddz); out.dqz.append((dqx, dqy))
    inf = torch.full_like(zd, math.inf)
    cand = torch.stack([torch.where(out.valid[s] & live0, out.e_s[s].detach(), inf) for s in range(S)])          # [S,H,W]
    best, arg = cand.min(0)                          # torch.min returns the FIRST index of a tie: the lowest s
    for s in range(S - 1, -1, -1):                   # (made explicit all the same)
        arg = torch.where(cand[s] == best, torch.full_like(arg, s), arg)
    live = torch.isfinite(best)
    src = torch.where(live, arg, torch.full_like(arg, -1))
    pick = lambda lst: torch.stack(list(lst)).gather(0, arg[None])[0]
    e_live = torch.where(live, pick(out.e_s), torch.zeros_like(zd))
    n = float(live.sum())
    loss = w * e_live.sum() / max(n, 1.0)
    with torch.no_grad():
        dz = torch.where(live, pick(out.dz_s), torch.zeros_like(zd))
        scale = w / max(n, 1.0)
        ad = torch.where(live, a.detach(), one)
        out.g_depth = torch.where(live, scale * dz / ad, torch.zeros_like(zd))
        out.g_alpha = torch.where(live, -scale * dz * zd / ad, torch.zeros_like(zd))
        out.dz, out.e, out.src, out.live, out.live0, out.n_live = dz, e_live.detach(), src, live, live0, n
        out.loss = float(loss)
        n0 = float((src == 0).sum())
        out.parts = [float(loss), float(e_live.sum()) / max(n, 1.0), n / (H * W), n0 / max(n, 1.0)]
        out.de = torch.where(live, pick(out.de_s), torch.zeros_like(zd))
        out.ddz = torch.where(live, pick(out.ddz_s), torch.zeros_like(zd))
        out.cand, out.z, out.a = cand, zd, a.detach()
    if autograd:
        out.ag_depth, out.ag_alpha = torch.autograd.grad(loss, (D, a), allow_unused=True)
        out.ag_depth = torch.zeros_like(zd) if out.ag_depth is None else out.ag_depth
        out.ag_alpha = torch.zeros_like(zd) if out.ag_alpha is None else out.ag_alpha
    return out


def kinks(r, skip_flat_lattice=False):
    """From a `term` result: (ambiguous [H,W], unsure [H,W]) - the pixels the per-pixel comparison leaves out, by the margins of the
    module docstring (each SAFETY x the first-order fp32 error of the quantity concerned):
      ambiguous: the live / dead state or the chosen source may differ in fp32 - for ANY source of a pixel that is live by its alpha
                 and depth, q within its |dq| of the validity border (0, W-1, 0, H-1) or X_z within its |dX_z| of 0.01; or the two
                 smallest e_s closer than the sum of their |de_s|.  (a against alpha_min and D against 0 are comparisons of the
                 shared fp32 inputs themselves: exact, margin 0.)
      unsure:    the gradient may differ - q of the CHOSEN source within |dq| of a lattice line (the bilinear cell changes), or a
                 channel difference of the chosen source within its |dI| of 0 (the sign flips).
    `skip_flat_lattice`: a lattice line of one axis is no kink where dq/dz along THAT axis is negligible - crossing a y lattice line
    changes dI/dq_y alone (dI/dq_x is continuous across it), by at most 2 for images in [0, 1], and dI/dq_y enters the unscaled dL/dz
    times dq_y/dz: where 2 |dq_y/dz| is within the error model's own figure for dL/dz the line is not flagged.  Cameras on an x
    baseline with equal intrinsics have q_y = y on EVERY pixel and dq_y/dz = 0 up to the rounding of the float64 inverse (the trainer's
    synthetic scene): without this every pixel would be flagged."""
    H, W, S = r.H, r.W, r.S
    amb = torch.zeros(H, W, dtype=torch.bool)
    for s in range(S):
        (qx, qy), (dqx, dqy), Xz = r.q[s], r.dq[s], r.Xz[s]
        mx, my = SAFETY * dqx, SAFETY * dqy
        near = (qx.abs() <= mx) | ((qx - (W - 1)).abs() <= mx) | (qy.abs() <= my) | ((qy - (H - 1)).abs() <= my)
        # |dX_z| <= |z| |dA_z| + 3 U (|z A_z| + |t_z|) <= 9 U (|X_z| + 2 |t_z|) here: bounded by 32 U (|X_z| + 1) for the cases' |t| <= 1.5
        near |= (Xz - ZNEAR).abs() <= SAFETY * 32 * U * (Xz.abs() + 1.0)
        near |= ~torch.isfinite(qx) | ~torch.isfinite(qy)
        amb |= near & r.live0
    if S > 1:
        de = torch.stack([torch.where(torch.isfinite(r.cand[s]), r.de_s[s], torch.zeros_like(r.de_s[s])) for s in range(S)])
        order = r.cand.argsort(0)
        c2, d2 = r.cand.gather(0, order[:2]), de.gather(0, order[:2])
        amb |= torch.isfinite(c2[1]) & ((c2[1] - c2[0]) <= SAFETY * (d2[0] + d2[1]))
    unsure = torch.zeros(H, W, dtype=torch.bool)
    arg = r.src.clamp(min=0)
    for s in range(S):
        (qx, qy), (dqx, dqy) = r.q[s], r.dq[s]
        lat_x, lat_y = (qx - qx.round()).abs() <= SAFETY * dqx, (qy - qy.round()).abs() <= SAFETY * dqy
        if skip_flat_lattice:
            lat_x, lat_y = lat_x & (2 * r.dqz[s][0].abs() > r.ddz_s[s]), lat_y & (2 * r.dqz[s][1].abs() > r.ddz_s[s])
        lat = lat_x | lat_y
        flip = (r.diff[s].abs() <= SAFETY * (r.dval[s] + U * r.diff[s].abs())).any(0)
        unsure |= (arg == s) & r.live & (lat | flip)
    return amb, unsure


# ---------------------------------------------------------------------------------------------------------------- shared cases
def smooth_image(H, W, gen, noise=0.01):
    """[3,H,W] fp32 in about [0.1, 0.9]: three low-frequency sinusoids per channel plus small noise"""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64) / max(H - 1, 1), torch.arange(W, dtype=F64) / max(W - 1, 1), indexing="ij")
    img = torch.full((3, H, W), 0.5, dtype=F64)
    for c in range(3):
        for _ in range(3):
            kx, ky = (torch.rand(2, generator=gen, dtype=F64) * 3.0 - 1.5) * 2 * math.pi
            ph = torch.rand(1, generator=gen, dtype=F64) * 2 * math.pi
            img[c] += 0.12 * torch.sin(kx * xs + ky * ys + ph)
    img += noise * torch.randn(3, H, W, generator=gen, dtype=F64)
    return img.clamp(0.02, 0.98).to(torch.float32)


def case_intrinsics(H, W):
    f = W / (2 * math.tan(math.radians(30)))
    return np.array([f, f, (W - 1) / 2, (H - 1) / 2], dtype=np.float64)


def make_case(H, W, S, seed):
    """Inputs of one comparison case: smooth images, a smooth depth around 3 with noise, an alpha field that dips below alpha_min
    and reaches 0 in places, and S relative poses (a small rotation and a translation that moves about a third of the image out of
    each source: the validity border crosses the image)."""
    gen = torch.Generator().manual_seed(seed)
    k = case_intrinsics(H, W)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64) / max(H - 1, 1), torch.arange(W, dtype=F64) / max(W - 1, 1), indexing="ij")
    z0 = 3.0
    z = z0 * (1.0 + 0.15 * torch.sin(2.1 * xs + 1.3 * ys + 0.4) + 0.01 * torch.randn(H, W, generator=gen, dtype=F64))
    alpha = (0.8 + 0.35 * torch.sin(5.0 * xs - 3.0 * ys + 1.0) + 0.02 * torch.randn(H, W, generator=gen, dtype=F64)).clamp(0.0, 1.0)
    alpha = torch.where(alpha < 0.3, torch.zeros_like(alpha), alpha)
    table = np.zeros((S, 16), dtype=np.float64)
    shifts = [(0.3, 0.02), (-0.25, -0.03), (0.04, 0.3), (-0.05, -0.2)]
    for s in range(S):
        sx, sy = shifts[s]
        th = 0.03 * (1 if s % 2 == 0 else -1)
        R = np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]])
        t = np.array([sx * W * z0 / k[0], sy * H * z0 / k[1], 0.05 * (s + 1)])
        table[s] = np.concatenate([R.reshape(9), t, k])
    return dict(depth=(z * alpha).to(torch.float32), alpha=alpha.to(torch.float32), target=smooth_image(H, W, gen),
                sources=[smooth_image(H, W, gen) for _ in range(S)], views=(k.astype(np.float32), table.astype(np.float32)), H=H, W=W, S=S)


# the kernel's grid cap (csrc/reproj.hip: kRpMaxBlocks blocks of kRpThreads threads, one group of four pixels per thread and trip)
MAX_BLOCKS, THREADS = 1024, 256


def trips(H, W):
    groups = H * ((W + 3) // 4)
    blocks = min(-(-groups // THREADS), MAX_BLOCKS)
    return -(-groups // (blocks * THREADS))


SECOND_TRIP = (1025, 1024)       # the first H at W = 1024 whose H * W / 4 groups exceed MAX_BLOCKS * THREADS: two trips
# (H, W, S, seed): the seeds are fixed after tests/test_reproj_cpu.py showed the reference's own left-out share inside 2 % (none at
# all for the two smallest shapes)
CASES = [(2, 2, 1, 3), (3, 5, 2, 1), (37, 53, 1, 1), (37, 53, 2, 2), (37, 53, 4, 3), (64, 257, 2, 4), (64, 257, 4, 5), (36, 52, 4, 9)]
BIG_CASE = SECOND_TRIP + (1, 6)
MAX_LEFT_OUT = 0.02

_cache = {}


def reference(case_key, weight=1.0, alpha_min=0.5):
    """(case, term result, (ambiguous, unsure)) of one of CASES / BIG_CASE: computed once, shared, left unchanged"""
    key = (tuple(case_key), weight, alpha_min)
    if key not in _cache:
        c = make_case(*case_key)
        r = term(c["depth"], c["alpha"], c["target"], c["sources"], c["views"], weight, alpha_min)
        _cache[key] = (c, r, kinks(r))
    return _cache[key]


# ---------------------------------------------------------------------------------------------------- the abstract descent design
def plane_design(H=24, W=64, baseline=0.8, tilt=0.25, z_mid=2.0, start=1.08, cycles_in_error=0.2):
    """A textured tilted plane seen by three cameras on an x baseline (identity rotations), images in closed form by ray-plane
    intersection.  Plane: Z = z_mid + tilt X in the MIDDLE camera's frame (the target).  The texture is a sum of sinusoids of the
    plane's X and Y per channel whose wavelength comes from the initial disparity error: starting at z = `start` z*, a pixel's
    reprojection is fx b |1/z - 1/z*| pixels off; the texture's shortest wavelength, seen in the image, is that error divided by
    `cycles_in_error` (0.2: the start sits well inside the basin of the L1 residual's minimum, under a quarter wave).
    -> dict(target, sources, views, z_true [H,W], z_start, all float64-exact closed forms stored as fp32 where the operator needs them)"""
    k = case_intrinsics(H, W)
    fx, fy, cx, cy = k
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")

    def plane_hit(cam_x):
        """pixel grid of a camera at world x = cam_x (middle camera's frame = world) -> plane point (X, Y, Z) in the world and depth"""
        rx, ry = (xs - cx) / fx, (ys - cy) / fy
        # (cam_x + z rx, z ry, z) on Z = z_mid + tilt X  ->  z = (z_mid + tilt cam_x) / (1 - tilt rx)
        z = (z_mid + tilt * cam_x) / (1.0 - tilt * rx)
        return cam_x + z * rx, z * ry, z

    _, _, z_true = plane_hit(0.0)
    err_px = fx * baseline * (1.0 - 1.0 / start) / z_true.min()
    lam_px = err_px / cycles_in_error
    lam = lam_px * z_mid / fx                        # wavelength on the plane
    om = 2 * math.pi / lam

    def texture(X, Y):
        chans = []
        for c in range(3):
            chans.append(0.5 + 0.2 * np.sin(om * X + 0.7 * c) + 0.15 * np.sin(0.6 * om * Y + 0.5 * om * X + 1.1 * c)
                         + 0.1 * np.sin(0.35 * om * (X - Y) + 0.3 * c))
        return np.stack(chans)

    image = lambda cam_x: texture(*plane_hit(cam_x)[:2])
    table = np.zeros((2, 16), dtype=np.float64)
    for s, b in enumerate((-baseline, baseline)):
        # source camera at world x = b: X_s = X_t - (b, 0, 0)
        table[s] = np.concatenate([np.eye(3).reshape(9), [-b, 0.0, 0.0], k])
    f32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32))
    return dict(target=f32(image(0.0)), sources=[f32(image(-baseline)), f32(image(baseline))],
                views=(k.astype(np.float32), table.astype(np.float32)), z_true=torch.as_tensor(z_true), z_start=torch.as_tensor(start * z_true),
                H=H, W=W, lam_px=lam_px, err_px=err_px)


DESCENT_ITERS = 150


def descent_rate(design):
    """The fixed step of the plain gradient descent, from the design alone (float64): with weight = H W the per-pixel gradient is
    un-normalised; the step moves a pixel by 1/40 of the initial depth error per iteration at the mean initial gradient magnitude."""
    H, W = design["H"], design["W"]
    z0 = design["z_start"]
    r = term(z0.to(torch.float32), torch.ones(H, W), design["target"], design["sources"], design["views"], float(H * W), 0.5)
    g = r.g_depth.abs()
    return float((z0 - design["z_true"]).abs().mean() / (40.0 * g[r.live].mean()))


def descend(design, step_fn, lr, iters=DESCENT_ITERS):
    """Plain gradient descent on a per-pixel z with alpha = 1: z <- z - lr * g_depth(z); `step_fn(z fp32 [H,W]) -> g_depth [H,W]`.
    The iterate is kept in float64 on the CPU and handed over as fp32.  -> (final z, mean |z - z*| at the start, at the end)"""
    z = design["z_start"].clone()
    zt = design["z_true"]
    e0 = float((z - zt).abs().mean())
    for _ in range(iters):
        z = z - lr * step_fn(z.to(torch.float32)).to(F64).cpu()
    return z, e0, float((z - zt).abs().mean())


def ref_step(design):
    H, W = design["H"], design["W"]
    ones = torch.ones(H, W)
    return lambda z32: term(z32, ones, design["target"], design["sources"], design["views"], float(H * W), 0.5).g_depth
