"""The patch-wise depth-correlation term (csrc/depth_loss.hip, train_ops.depth_correlation_local_loss[_step]) restated in float64
as a plain loop over patches.  A helper module, not a test: tests/test_depth_local_cpu.py and tests/test_depth_local_gpu.py use it.

For an H x W depth d and prior p, patch size P and origin (oy, ox), 0 <= oy, ox < P: patch (i, j) covers rows oy + iP .. oy +
(i+1)P - 1 and columns ox + jP .. ox + (j+1)P - 1; only the K = floor((H - oy) / P) * floor((W - ox) / P) patches inside the image
count.  Per patch the global term's rules (tests/test_depth_loss_gpu.py::ref_dcorr): r_A = Pearson(d, -p), r_B = Pearson(d, 1 / (p +
offset)) from centred sums, clamped to [-1, 1]; a flat d or t gives r = 0, loss 1 and a zero gradient; L_k = min(1 - r_A, 1 - r_B),
A on a tie.  L = weight / K * sum_k L_k; dL/dd = weight / K * (the per-patch gradient) inside patch k and 0 in no full patch."""
import torch


def grid(H, W, P, oy, ox):
    """(PY, PX): full patches down and across"""
    return (H - oy) // P, (W - ox) // P


def _branch(d, t):
    """(r, d(1 - r)/dd) of one patch and one transform; r = 0 and a zero gradient for a flat d or t"""
    if float(d.max()) == float(d.min()) or float(t.max()) == float(t.min()):
        return 0.0, torch.zeros_like(d), True
    dc, tc = d - d.mean(), t - t.mean()
    sdd, stt, sdt = (dc * dc).sum(), (tc * tc).sum(), (dc * tc).sum()
    s = torch.sqrt(sdd * stt)
    r = float((sdt / s).clamp(-1.0, 1.0))
    return r, -(tc / s - r * dc / sdd), False


def ref_local(depth, prior, weight=1.0, patch=32, origin=(0, 0), offset=200.0, mode="min"):
    """-> dict(loss, grad [H,W] float64, parts [4], and per patch [PY,PX]: lk, r, branch, flat, gap = |L_A - L_B|, gmax = the largest
    |gradient entry| of the patch)"""
    d = depth.detach().double().cpu().reshape(depth.shape[-2:])
    p = prior.detach().double().cpu().reshape(prior.shape[-2:])
    H, W = d.shape
    P, (oy, ox) = int(patch), origin
    PY, PX = grid(H, W, P, oy, ox)
    K = PY * PX
    assert K >= 1
    grad = torch.zeros(H, W, dtype=torch.float64)
    per = {k: torch.zeros(PY, PX, dtype=torch.float64) for k in ("lk", "r", "branch", "flat", "gap", "gmax")}
    for i in range(PY):
        for j in range(PX):
            ys, xs = slice(oy + i * P, oy + (i + 1) * P), slice(ox + j * P, ox + (j + 1) * P)
            dd, pp = d[ys, xs].reshape(-1), p[ys, xs].reshape(-1)
            ra, ga, fa = _branch(dd, -pp)
            rb, gb, fb = _branch(dd, 1.0 / (pp + offset)) if mode != "A" else (0.0, torch.zeros_like(dd), True)
            la, lb = 1.0 - ra, 1.0 - rb
            use_b = mode == "B" or (mode == "min" and lb < la)
            g = (gb if use_b else ga) * (weight / K)
            grad[ys, xs] = g.reshape(P, P)
            per["lk"][i, j] = lb if use_b else la
            per["r"][i, j] = rb if use_b else ra
            per["branch"][i, j] = float(use_b)
            per["flat"][i, j] = float(fb if use_b else fa)
            per["gap"][i, j] = abs(la - lb)
            per["gmax"][i, j] = float(g.abs().max())
    loss = weight / K * float(per["lk"].sum())
    parts = [loss, float(per["r"].mean()), float(per["branch"].mean()), float(per["flat"].mean())]
    return dict(loss=loss, grad=grad, parts=parts, K=K, **per)


def ref_local_torch(d, p, weight, patch, origin=(0, 0), offset=200.0):
    """The same term (mode "min") as a differentiable float64 torch expression of d [.., H, W], for the oracle training step."""
    d = d.reshape(d.shape[-2:])
    p = p.reshape(p.shape[-2:]).to(d.dtype)
    H, W = d.shape
    P, (oy, ox) = int(patch), origin
    PY, PX = grid(H, W, P, oy, ox)

    def one_minus_r(x, t):
        if float(x.detach().max()) == float(x.detach().min()) or float(t.max()) == float(t.min()):
            return torch.ones((), dtype=x.dtype)
        xc, tc = x - x.mean(), t - t.mean()
        return 1.0 - ((xc * tc).sum() / torch.sqrt((xc * xc).sum() * (tc * tc).sum())).clamp(-1.0, 1.0)

    total = torch.zeros((), dtype=d.dtype)
    for i in range(PY):
        for j in range(PX):
            ys, xs = slice(oy + i * P, oy + (i + 1) * P), slice(ox + j * P, ox + (j + 1) * P)
            x, q = d[ys, xs].reshape(-1), p[ys, xs].reshape(-1)
            la, lb = one_minus_r(x, -q), one_minus_r(x, 1.0 / (q + offset))
            total = total + (lb if float(lb.detach()) < float(la.detach()) else la)
    return weight / (PY * PX) * total


def patch_of(H, W, P, oy, ox):
    """int64 [H,W]: the flat index i * PX + j of the full patch a pixel lies in, -1 in none"""
    PY, PX = grid(H, W, P, oy, ox)
    y, x = torch.arange(H)[:, None], torch.arange(W)[None, :]
    i, j = torch.div(y - oy, P, rounding_mode="floor"), torch.div(x - ox, P, rounding_mode="floor")
    ok = (y >= oy) & (x >= ox) & (i < PY) & (j < PX)
    return torch.where(ok, i * PX + j, torch.full((H, W), -1))
