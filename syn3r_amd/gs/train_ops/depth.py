"""The depth terms of the trainer on the HIP library: FSGS' depth correlation against a monocular prior, whole-map and patch-wise
(csrc/depth_loss.hip), and the prior-free edge-aware smoothness (csrc/depth_smooth.hip), each as an autograd operator and as a `*_step`
function without autograd.  The autograd route is ONE Function for the three: a `_Term` row and an argument function say what differs.
The `*_step` functions are spelled out per term: they sit in the trainer's explicit step, where a shared body's extra call level and
tuple traffic showed as 0.2 - 0.6 us per call (profiles/r21/train_ops_split.txt)."""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from ... import _lib as L

_DCORR_MODES = {"min": 0, "A": 1, "B": 2}      # SYN3R_DCORR_MIN / _A / _B


def _hw(t: torch.Tensor):
    """The ONE shape rule of a depth map or prior: (H, W) of a [1,H,W] or [H,W] tensor, else None."""
    return tuple(t.shape[1:]) if t.dim() == 3 and t.shape[0] == 1 else (tuple(t.shape) if t.dim() == 2 else None)


def _prior_pair(who: str, depth: torch.Tensor, prior: torch.Tensor, mode: str):
    """(depth, prior) as contiguous fp32 tensors and the mode tag; depth [1,H,W] or [H,W], prior [H,W] or [1,H,W]."""
    L.require_gpu(depth, prior)
    if depth.dtype != torch.float32 or prior.dtype != torch.float32:
        raise ValueError(f"{who}: depth and prior must be float32")
    if _hw(depth) is None or _hw(prior) is None or _hw(depth) != _hw(prior):
        raise ValueError(f"{who}: depth [1,H,W] or [H,W] and prior [H,W] or [1,H,W] of the same H, W; got "
                         f"{tuple(depth.shape)} and {tuple(prior.shape)}")
    if mode not in _DCORR_MODES:
        raise ValueError(f"{who}: mode must be one of {sorted(_DCORR_MODES)}, got {mode!r}")
    return depth.detach().contiguous(), prior.detach().contiguous(), _DCORR_MODES[mode]


def _local_pair(who: str, depth: torch.Tensor, prior: torch.Tensor, patch: int, origin, mode: str):
    """`_prior_pair` plus the patch grid: -> (depth, prior, mode tag, (H, W, P, oy, ox)).  The grid's own limits (P in [2, 256], the
    origin in [0, P), at least one full patch) are the library's to reject."""
    d, p, m = _prior_pair(who, depth, prior, mode)
    try:
        oy, ox = (int(v) for v in origin)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: origin must be a pair (oy, ox) of integers, got {origin!r}") from None
    H, W = (int(v) for v in d.shape[-2:])
    return d, p, m, (H, W, int(patch), oy, ox)


def _smooth_pair(who: str, depth: torch.Tensor, weights: torch.Tensor):
    """(depth, weights) as contiguous fp32 tensors (a view at any 4-byte offset is taken as it is: the library picks its scalar
    path) and (H, W); depth [1,H,W] or [H,W], weights [2,H,W]."""
    L.require_gpu(depth, weights)
    if depth.dtype != torch.float32 or weights.dtype != torch.float32:
        raise ValueError(f"{who}: depth and weights must be float32")
    hw = _hw(depth)
    if hw is None or weights.dim() != 3 or tuple(weights.shape) != (2,) + hw:
        raise ValueError(f"{who}: depth [1,H,W] or [H,W] and weights [2,H,W] of the same H, W; got {tuple(depth.shape)} and "
                         f"{tuple(weights.shape)}")
    return depth.detach().contiguous(), weights.detach().contiguous(), (int(hw[0]), int(hw[1]))


# For `_DepthTerm`, one per term: the user's arguments -> (depth, other, head); `head`: the scalars of the entries between the two
# pointers and `grad_loss`, in the entry's order.
def _global_args(who: str, depth, prior, weight, offset, mode):
    d, p, m = _prior_pair(who, depth, prior, mode)
    return d, p, (d.numel(), float(weight), float(offset), m)


def _local_args(who: str, depth, prior, weight, patch, origin, offset, mode):
    d, p, m, geom = _local_pair(who, depth, prior, patch, origin, mode)
    return d, p, (*geom, float(weight), float(offset), m)


def _smooth_args(who: str, depth, weights, weight):
    d, w, hw = _smooth_pair(who, depth, weights)
    return d, w, (*hw, float(weight))


class _Term(NamedTuple):
    """What `_DepthTerm` knows of a term; its entries are `syn3r_<stem>` and `syn3r_<stem>_backward`."""
    stem: str
    workspace_bytes: str    # the size function, which takes the first `n_geom` scalars of the head
    n_geom: int
    accumulate: bool        # the backward entry takes `accumulate` (and the term's step function a `grad_out`)
    args: Callable          # (who, depth, other, *the user's other arguments) -> (depth, other, head)


_GLOBAL = _Term("depth_corr_loss", "syn3r_depth_corr_loss_workspace_bytes", 1, False, _global_args)
_LOCAL = _Term("depth_corr_local_loss", "syn3r_depth_corr_local_workspace_bytes", 5, True, _local_args)
_SMOOTH = _Term("depth_smooth_loss", "syn3r_depth_smooth_workspace_bytes", 2, True, _smooth_args)


def _term_forward(term: _Term, d: torch.Tensor, other: torch.Tensor, head: tuple):
    """The `<stem>` entry: -> (parts [4], the workspace it filled)."""
    lib = L.load()
    # own buffer, not the shared workspace cache: what the statistics pass leaves must survive until backward
    ws = torch.empty(max(getattr(lib, term.workspace_bytes)(*head[:term.n_geom]), 256), dtype=torch.uint8, device=d.device)
    parts = torch.empty(4, dtype=torch.float32, device=d.device)
    L.check(getattr(lib, "syn3r_" + term.stem)(L.ptr(d), L.ptr(other), *head, L.ptr(parts), L.ptr(ws), ws.numel(),
                                               L.stream_ptr(d.device)), term.stem)
    return parts, ws


class _DepthTerm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, term: _Term, who: str, depth: torch.Tensor, other: torch.Tensor, *user):
        d, other, head = term.args(who, depth, other, *user)
        parts, ws = _term_forward(term, d, other, head)
        ctx.save_for_backward(d, other, ws)
        ctx.args = (term, head, depth.shape, len(user))
        ctx.mark_non_differentiable(parts)
        return parts[0].clone(), parts

    @staticmethod
    def backward(ctx, grad_loss: torch.Tensor, _grad_parts):
        L.join_active_trace()
        d, other, ws = ctx.saved_tensors
        term, head, shape, n_user = ctx.args
        go = grad_loss.to(torch.float32).contiguous()
        grad = torch.empty_like(d)
        accumulate = (0,) if term.accumulate else ()
        L.check(getattr(L.load(), f"syn3r_{term.stem}_backward")(L.ptr(d), L.ptr(other), *head, L.ptr(go), L.ptr(ws), ws.numel(),
                                                                 L.ptr(grad), *accumulate, L.stream_ptr(d.device)),
                term.stem + "_backward")
        return (None, None, grad.reshape(shape), None) + (None,) * n_user


def _check_grad_out(who: str, d: torch.Tensor, grad_out: torch.Tensor, name: str = "grad_out") -> None:
    """A step function's `grad_out` (or the buffer `name`): float32, contiguous, depth's number of elements, on its device."""
    L.require_gpu(d, grad_out)
    if grad_out.dtype != torch.float32 or grad_out.numel() != d.numel() or not grad_out.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous float32 tensor of depth's {d.numel()} elements")


def depth_correlation_loss(depth: torch.Tensor, prior: torch.Tensor, weight: float = 1.0, offset: float = 200.0, mode: str = "min",
                           return_parts: bool = False):
    """FSGS' depth-correlation term (Zhu et al., ECCV 2024, "geometry guidance") on one rendered depth map and a monocular prior:
    `weight * min(1 - r_A, 1 - r_B)`, r = Pearson(depth, t) for t = -prior (A) and t = 1 / (prior + offset) (B); `mode` "A" / "B"
    keeps one branch.  The two-branch minimum and offset 200 are recalled from FSGS' train.py (not available): UNPINNED.  A flat
    render or prior gives r = 0 (loss = weight) and a zero gradient, not NaN.  Device scalar, no host synchronisation; backward is
    the kernel's gradient pass through the chosen branch (csrc/depth_loss.hip).  `return_parts`: also the device tensor
    [loss, r_A, r_B, branch (0 = A, 1 = B)]."""
    loss, parts = _DepthTerm.apply(_GLOBAL, "depth_correlation_loss", depth, prior, weight, offset, mode)
    return (loss, parts) if return_parts else loss


def depth_correlation_loss_step(depth: torch.Tensor, prior: torch.Tensor, weight: float = 1.0, offset: float = 200.0,
                                mode: str = "min", grad_loss: torch.Tensor = None, return_parts: bool = False):
    """Value AND depth gradient of `depth_correlation_loss` without autograd (`syn3r_depth_corr_loss_step`: two launches).  Returns
    (loss - a view of parts[0] -, grad_depth shaped like depth) [+ parts]; `grad_loss`: device scalar, default 1.  Same bits as
    the autograd Function's forward + backward."""
    d, p, m = _prior_pair("depth_correlation_loss_step", depth, prior, mode)
    dev = d.device
    lib = L.load()
    n = d.numel()
    ws = L.workspace(dev, lib.syn3r_depth_corr_loss_workspace_bytes(n), "dcorr_step")
    parts = torch.empty(4, dtype=torch.float32, device=dev)
    grad = torch.empty_like(d)
    go = grad_loss.to(torch.float32).contiguous() if grad_loss is not None else None
    L.check(lib.syn3r_depth_corr_loss_step(L.ptr(d), L.ptr(p), n, float(weight), float(offset), m, L.ptr(go), L.ptr(parts),
                                           L.ptr(grad), L.ptr(ws), ws.numel(), L.stream_ptr(dev)), "depth_corr_loss_step")
    return (parts[0], grad, parts) if return_parts else (parts[0], grad)


def depth_correlation_local_loss(depth: torch.Tensor, prior: torch.Tensor, weight: float = 1.0, patch: int = 32, origin=(0, 0),
                                 offset: float = 200.0, mode: str = "min", return_parts: bool = False):
    """The depth-correlation term PATCH-WISE (EXTENSION after SparseGS' patch-based Pearson / DNGaussian's local normalisation: a
    monocular prior is one monotone transform of the depth only locally): `weight / K * sum_k min(1 - r_A, 1 - r_B)` over the K
    `patch` x `patch` tiles of the grid with origin `origin` = (oy, ox), 0 <= oy, ox < patch, that lie inside the image, the
    branch and the flat rule of `depth_correlation_loss` taken per patch; pixels in no full patch have a zero gradient.  The two
    transforms and offset 200 are recalled (UNPINNED).  Device scalar, no host synchronisation; backward is the kernel's gradient pass
    (csrc/depth_loss.hip).  `return_parts`: also the device tensor [loss, mean chosen r, share of patches on B, share of flat patches]."""
    loss, parts = _DepthTerm.apply(_LOCAL, "depth_correlation_local_loss", depth, prior, weight, patch, origin, offset, mode)
    return (loss, parts) if return_parts else loss


def depth_correlation_local_loss_step(depth: torch.Tensor, prior: torch.Tensor, weight: float = 1.0, patch: int = 32, origin=(0, 0),
                                      offset: float = 200.0, mode: str = "min", grad_loss: torch.Tensor = None,
                                      grad_out: torch.Tensor = None, return_parts: bool = False):
    """Value AND depth gradient of `depth_correlation_local_loss` without autograd (`syn3r_depth_corr_local_loss_step`: two
    launches).  Returns (loss - a view of parts[0] -, grad_depth shaped like depth) [+ parts]; `grad_loss`: device scalar, default 1.
    `grad_out` (float32, contiguous, depth's number of elements, on its device): the gradient is ADDED to it inside the full patches,
    the rest is left alone, and it is what comes back; without it a new tensor with zeros outside the patches.  Same bits as the
    autograd Function's forward + backward."""
    who = "depth_correlation_local_loss_step"
    d, p, m, geom = _local_pair(who, depth, prior, patch, origin, mode)
    dev = d.device
    lib = L.load()
    if grad_out is not None:
        _check_grad_out(who, d, grad_out)
    ws = L.workspace(dev, lib.syn3r_depth_corr_local_workspace_bytes(*geom), "dcorr_local_step")
    parts = torch.empty(4, dtype=torch.float32, device=dev)
    grad = torch.empty_like(d) if grad_out is None else grad_out
    go = grad_loss.to(torch.float32).contiguous() if grad_loss is not None else None
    L.check(lib.syn3r_depth_corr_local_loss_step(L.ptr(d), L.ptr(p), *geom, float(weight), float(offset), m, L.ptr(go), L.ptr(parts),
                                                 L.ptr(grad), int(grad_out is not None), L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
            "depth_corr_local_loss_step")
    return (parts[0], grad, parts) if return_parts else (parts[0], grad)


def depth_correlation_local_records(depth: torch.Tensor, prior: torch.Tensor, patch: int = 32, origin=(0, 0), offset: float = 200.0,
                                    mode: str = "min") -> torch.Tensor:
    """The finished per-patch records of the patch-wise term as a float64 [PY, PX, 8] device tensor (diagnostics and tests): per
    patch [mean depth, mean of the chosen transform's variable, the two gradient coefficients for weight 1, L_k, the chosen r,
    branch (0 = A, 1 = B), flat (0 / 1)] - what `syn3r_depth_corr_local_loss` leaves at the head of its workspace."""
    d, p, head = _local_args("depth_correlation_local_records", depth, prior, 1.0, patch, origin, offset, mode)
    _, ws = _term_forward(_LOCAL, d, p, head)
    H, W, P, oy, ox = head[:5]
    PY, PX = (H - oy) // P, (W - ox) // P
    return ws[:PY * PX * 64].view(torch.float64).reshape(PY, PX, 8).clone()


def depth_edge_weights(image: torch.Tensor, gamma: float = 1.0) -> torch.Tensor:
    """The edge weights of the depth-smoothness term from a camera's target image [3,H,W] fp32 (`syn3r_depth_edge_weights`,
    csrc/depth_smooth.hip: one launch): [2,H,W] fp32, wx[y,x] = exp(-gamma mean_c |I_c[y,x+1] - I_c[y,x]|), wy the same downwards;
    zeros in the absent last column of wx and last row of wy.  gamma = 1 is recalled from Monodepth2: UNPINNED."""
    dev = L.require_gpu(image)
    if image.dim() != 3 or image.shape[0] != 3 or image.dtype != torch.float32:
        raise ValueError(f"depth_edge_weights: image must be a float32 [3,H,W] tensor, got {image.dtype} {tuple(image.shape)}")
    image = image.detach().contiguous()
    H, W = int(image.shape[1]), int(image.shape[2])
    out = torch.empty((2, H, W), dtype=torch.float32, device=dev)
    L.check(L.load().syn3r_depth_edge_weights(L.ptr(image), H, W, float(gamma), L.ptr(out), L.stream_ptr(dev)), "depth_edge_weights")
    return out


def depth_smoothness_loss(depth: torch.Tensor, weights: torch.Tensor, weight: float = 1.0, return_parts: bool = False):
    """Prior-free edge-aware smoothness of one rendered depth map (EXTENSION; Monodepth2's form): `weight * (S_x + S_y) / m`, m the
    mean depth, S_x the mean over the H (W - 1) horizontal pixel pairs of wx |d[y,x+1] - d[y,x]|, S_y the same over the (H - 1) W
    vertical ones with wy; `weights` = [wx, wy] from `depth_edge_weights` (their last column / row is never read).  The gradient goes
    through the mean; m <= 0 (an empty render) gives 0 and a zero gradient, not NaN.  The division by the mean is recalled from
    Monodepth2: UNPINNED.  Device scalar, no host synchronisation; backward is the kernel's gradient pass (csrc/depth_smooth.hip).
    `return_parts`: also the device tensor [loss, S_x, S_y, m]."""
    loss, parts = _DepthTerm.apply(_SMOOTH, "depth_smoothness_loss", depth, weights, weight)
    return (loss, parts) if return_parts else loss


def depth_smoothness_loss_step(depth: torch.Tensor, weights: torch.Tensor, weight: float = 1.0, grad_loss: torch.Tensor = None,
                               grad_out: torch.Tensor = None, return_parts: bool = False):
    """Value AND depth gradient of `depth_smoothness_loss` without autograd (`syn3r_depth_smooth_loss_step`: two launches).  Returns
    (loss - a view of parts[0] -, grad_depth shaped like depth) [+ parts]; `grad_loss`: device scalar, default 1.  `grad_out`
    (float32, contiguous, depth's number of elements, on its device): the gradient is ADDED to it, and it is what comes back;
    without it a new tensor, every pixel written.  Same bits as the autograd Function's forward + backward."""
    who = "depth_smoothness_loss_step"
    d, w, hw = _smooth_pair(who, depth, weights)
    dev = d.device
    lib = L.load()
    if grad_out is not None:
        _check_grad_out(who, d, grad_out)
    ws = L.workspace(dev, lib.syn3r_depth_smooth_workspace_bytes(*hw), "dsmooth_step")
    parts = torch.empty(4, dtype=torch.float32, device=dev)
    grad = torch.empty_like(d) if grad_out is None else grad_out
    go = grad_loss.to(torch.float32).contiguous() if grad_loss is not None else None
    L.check(lib.syn3r_depth_smooth_loss_step(L.ptr(d), L.ptr(w), *hw, float(weight), L.ptr(go), L.ptr(parts), L.ptr(grad),
                                             int(grad_out is not None), L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
            "depth_smooth_loss_step")
    return (parts[0], grad, parts) if return_parts else (parts[0], grad)
