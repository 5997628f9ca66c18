"""Float64 restatement of the edge-aware depth-smoothness term (csrc/depth_smooth.hip, include/syn3r_hip.h):

    wx[y,x] = exp(-gamma * mean_c |I_c[y,x+1] - I_c[y,x]|)      wy[y,x] = exp(-gamma * mean_c |I_c[y+1,x] - I_c[y,x]|)
    m    = mean of d
    S_x  = 1/N_x * sum_{y, x<W-1} wx[y,x] |d[y,x+1] - d[y,x]|      N_x = H (W-1)
    S_y  = 1/N_y * sum_{y<H-1, x} wy[y,x] |d[y+1,x] - d[y,x]|      N_y = (H-1) W
    loss = weight * (S_x + S_y) / m

`ref_smooth_torch` is the formula as torch operators (its gradient is plain autograd, sign(0) = 0 as torch.abs has it);
`ref_smooth` is the closed form the kernels implement, with the quantities the tests' error bounds are made of."""
import torch


def ref_weights(image: torch.Tensor, gamma: float) -> torch.Tensor:
    """[2,H,W] float64 from the image's own (fp32) values; zeros in the absent last column of wx and last row of wy"""
    I = image.detach().cpu().double()
    _, H, W = I.shape
    out = torch.zeros(2, H, W, dtype=torch.float64)
    if W > 1:
        out[0, :, :-1] = torch.exp(-gamma * (I[:, :, 1:] - I[:, :, :-1]).abs().mean(0))
    if H > 1:
        out[1, :-1, :] = torch.exp(-gamma * (I[:, 1:, :] - I[:, :-1, :]).abs().mean(0))
    return out


def ref_smooth_torch(d: torch.Tensor, weights: torch.Tensor, weight: float) -> torch.Tensor:
    """The loss as a differentiable float64 expression of d [H,W]; an empty render (m <= 0) is a zero that still depends on d"""
    H, W = d.shape
    w = weights.detach().double()
    m = d.mean()
    if not float(m.detach()) > 0.0:
        return (d * 0.0).sum()
    s = d.new_zeros(())
    if W > 1:
        s = s + (w[0, :, :-1] * (d[:, 1:] - d[:, :-1]).abs()).sum() / (H * (W - 1))
    if H > 1:
        s = s + (w[1, :-1, :] * (d[1:, :] - d[:-1, :]).abs()).sum() / ((H - 1) * W)
    return weight * s / m


def ref_smooth(d: torch.Tensor, weights: torch.Tensor, weight: float, grad_loss: float = 1.0) -> dict:
    """Closed form in float64 on d [H,W] (or [1,H,W]) and weights [2,H,W]: loss, sx, sy, m, grad [H,W], and for the bounds
    `edges` [H,W] = sum over a pixel's edges of w / (N m) and `mean_term` = (S_x + S_y) / (m^2 H W)."""
    d = d.detach().cpu().double()
    d = d[0] if d.dim() == 3 else d
    w = weights.detach().cpu().double()
    H, W = d.shape
    nx, ny = H * (W - 1), (H - 1) * W
    m = float(d.mean())
    zero = torch.zeros(H, W, dtype=torch.float64)
    gx, gy, ex, ey = zero.clone(), zero.clone(), zero.clone(), zero.clone()
    sx = sy = 0.0
    if nx > 0:
        diff, wx = d[:, 1:] - d[:, :-1], w[0, :, :-1]
        sx = float((wx * diff.abs()).sum()) / nx
        t = wx * torch.sign(diff) / nx
        gx[:, 1:] += t
        gx[:, :-1] -= t
        ex[:, 1:] += wx / nx
        ex[:, :-1] += wx / nx
    if ny > 0:
        diff, wy = d[1:, :] - d[:-1, :], w[1, :-1, :]
        sy = float((wy * diff.abs()).sum()) / ny
        t = wy * torch.sign(diff) / ny
        gy[1:, :] += t
        gy[:-1, :] -= t
        ey[1:, :] += wy / ny
        ey[:-1, :] += wy / ny
    if not m > 0.0:
        return dict(loss=0.0, sx=sx, sy=sy, m=m, grad=zero, edges=zero, mean_term=0.0, empty=True)
    mean_term = (sx + sy) / (m * m * H * W)
    grad = weight * grad_loss * ((gx + gy) / m - mean_term)
    return dict(loss=weight * (sx + sy) / m, sx=sx, sy=sy, m=m, grad=grad, edges=(ex + ey) / m, mean_term=mean_term, empty=False)
