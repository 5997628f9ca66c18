"""Fused trainer-loop operators on the HIP library: the photometric L1 loss and the Adam
update that `gsTrainer.training()/finetune()` (call sites `model/diffusionGS.py:139,1640`; FSGS submodule not
vendored) run as torch elementwise chains.  No CPU fallback: they raise `Syn3rError` without the extension."""
from __future__ import annotations

from typing import Iterable, List, NamedTuple, Optional

import torch

from .. import _lib as L


def _map_arg(who: str, weight_map: Optional[torch.Tensor], image: torch.Tensor) -> Optional[torch.Tensor]:
    """The per-pixel weight map of the `*_map` entries as a contiguous fp32 [H,W] tensor (None stays None): [H,W] or [1,H,W] of
    the image's H, W, float32, on the image's device, without a gradient - anything else is a ValueError."""
    if weight_map is None:
        return None
    if not isinstance(weight_map, torch.Tensor):
        raise ValueError(f"{who}: weight_map must be a tensor, got {type(weight_map).__name__}")
    hw = tuple(image.shape[-2:]) if image.dim() >= 2 else None
    m = weight_map[0] if weight_map.dim() == 3 and weight_map.shape[0] == 1 else weight_map
    if hw is None or m.dim() != 2 or tuple(m.shape) != hw:
        raise ValueError(f"{who}: weight_map must be [H,W] or [1,H,W] for the image's H, W = {hw}; got {tuple(weight_map.shape)}")
    if m.dtype != torch.float32:
        raise ValueError(f"{who}: weight_map must be float32, got {m.dtype}")
    if m.device != image.device:
        raise ValueError(f"{who}: weight_map is on {m.device}, the image on {image.device}")
    if m.requires_grad:
        raise ValueError(f"{who}: weight_map is data - a map that requires grad is not supported")
    return m.contiguous()


def _l1_entries(lib, wm: Optional[torch.Tensor]):
    """The ONE place that knows the L1 loss has `_map` entries: -> (forward entry, backward entry, their name for `L.check`, and
    what a map adds to their argument lists: its pointer after `target`, its length after `n`; two empty tuples without one)"""
    if wm is None:
        return lib.syn3r_l1_loss, lib.syn3r_l1_loss_backward, "l1_loss", (), ()
    return lib.syn3r_l1_loss_map, lib.syn3r_l1_loss_map_backward, "l1_loss_map", (L.ptr(wm),), (wm.numel(),)


def _l1_forward(image: torch.Tensor, target: torch.Tensor, weight: float, weight_map: Optional[torch.Tensor] = None):
    L.require_gpu(image, target)
    if image.shape != target.shape or image.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError("l1_loss: image and target must be float32 tensors of the same shape")
    wm = _map_arg("l1_loss", weight_map, image)
    image, target = image.contiguous(), target.contiguous()
    lib = L.load()
    n = image.numel()
    loss = torch.empty((), dtype=torch.float32, device=image.device)
    ws = L.workspace(image.device, lib.syn3r_l1_loss_workspace_bytes(n), "l1")
    forward, _, name, map_ptr, map_len = _l1_entries(lib, wm)
    L.check(forward(L.ptr(image), L.ptr(target), *map_ptr, n, *map_len, float(weight), L.ptr(loss), L.ptr(ws), ws.numel(),
                    L.stream_ptr(image.device)), name)
    return loss, image, target, wm


def _l1_backward(image: torch.Tensor, target: torch.Tensor, weight: float, grad_loss, wm: Optional[torch.Tensor] = None):
    go = grad_loss.to(torch.float32).contiguous() if grad_loss is not None else None      # device scalar; None = 1
    grad = torch.empty_like(image)
    _, backward, name, map_ptr, map_len = _l1_entries(L.load(), wm)
    L.check(backward(L.ptr(image), L.ptr(target), *map_ptr, image.numel(), *map_len, float(weight), L.ptr(go), L.ptr(grad),
                     L.stream_ptr(image.device)), name + "_backward")
    return grad


class _L1Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image: torch.Tensor, target: torch.Tensor, weight: float, weight_map: Optional[torch.Tensor] = None):
        loss, image, target, wm = _l1_forward(image, target, weight, weight_map)
        ctx.save_for_backward(image, target)
        ctx.weight = float(weight)
        ctx.wm = wm                                   # data without a gradient: kept beside the saved tensors
        return loss

    @staticmethod
    def backward(ctx, grad_loss: torch.Tensor):
        L.join_active_trace()
        image, target = ctx.saved_tensors
        return _l1_backward(image, target, ctx.weight, grad_loss, ctx.wm), None, None, None


def l1_loss_step(image: torch.Tensor, target: torch.Tensor, weight: float = 1.0, grad_loss: torch.Tensor = None,
                 weight_map: Optional[torch.Tensor] = None):
    """Value and image gradient of `l1_loss` without autograd (the two launches `_L1Loss` makes): (loss, grad_image)."""
    loss, image, target, wm = _l1_forward(image.detach(), target.detach(), weight, weight_map)
    return loss, _l1_backward(image, target, weight, grad_loss, wm)


def l1_loss(image: torch.Tensor, target: torch.Tensor, weight: float = 1.0, weight_map: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`weight * (image - target).abs().mean()` as one read of both images (forward) and one read + one write
    (backward); the upstream gradient stays on the device.
    `weight_map` (EXTENSION, not in the reference; default None = the loss above): a per-pixel weight m, [H,W] or [1,H,W] fp32 on
    the image's device, shared by the channels of a [...,H,W] image: `weight * (m * (image - target).abs()).mean()` - the mean still
    over all elements, so a constant map k is the weight k * weight.  The map is data: no gradient, `requires_grad` is a ValueError."""
    return _L1Loss.apply(image, target, weight, weight_map)


def _photo_args(who: str, image: torch.Tensor, target: torch.Tensor, weight_map: Optional[torch.Tensor]):
    dev = L.require_gpu(image, target)
    if image.shape != target.shape or image.dim() != 3 or image.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f"{who}: image and target must be float32 [C,H,W] tensors of the same shape")
    return dev, _map_arg(who, weight_map, image)


def _photo_entries(lib, wm: Optional[torch.Tensor]):
    """The ONE place that knows the photometric loss has `_map` entries: -> (forward, backward and step entry, the workspace-size
    function, the length of `parts` (3: [loss, L1, SSIM]; 4 with a map: + mean(m)), their name for `L.check`, and what a map adds to
    their argument lists: its pointer after `target`; an empty tuple without one)"""
    if wm is None:
        return (lib.syn3r_photo_loss, lib.syn3r_photo_loss_backward, lib.syn3r_photo_loss_step, lib.syn3r_photo_loss_workspace_bytes,
                3, "photo_loss", ())
    return (lib.syn3r_photo_loss_map, lib.syn3r_photo_loss_map_backward, lib.syn3r_photo_loss_map_step,
            lib.syn3r_photo_loss_map_workspace_bytes, 4, "photo_loss_map", (L.ptr(wm),))


class _PhotoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image: torch.Tensor, target: torch.Tensor, lambda_dssim: float, weight: float,
                weight_map: Optional[torch.Tensor] = None):
        _, wm = _photo_args("photometric_loss", image, target, weight_map)
        image, target = image.contiguous(), target.contiguous()
        lib = L.load()
        C_, H_, W_ = image.shape
        forward, _, _, workspace_bytes, n_parts, name, map_ptr = _photo_entries(lib, wm)
        # own buffer, not the shared workspace cache: the derivative maps must survive until backward
        ws = torch.empty(workspace_bytes(C_, H_, W_), dtype=torch.uint8, device=image.device)
        out = torch.empty(n_parts, dtype=torch.float32, device=image.device)
        L.check(forward(L.ptr(image), L.ptr(target), *map_ptr, C_, H_, W_, float(lambda_dssim), float(weight), L.ptr(out), L.ptr(ws),
                        ws.numel(), L.stream_ptr(image.device)), name)
        ctx.save_for_backward(image, target, ws)
        ctx.args = (float(lambda_dssim), float(weight))
        ctx.wm = wm                                   # data without a gradient: kept beside the saved tensors
        ctx.mark_non_differentiable(out)
        ctx.parts = out
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, grad_loss: torch.Tensor, _grad_parts):
        L.join_active_trace()
        image, target, ws = ctx.saved_tensors
        lam, weight = ctx.args
        C_, H_, W_ = image.shape
        go = grad_loss.to(torch.float32).contiguous()
        grad = torch.empty_like(image)
        _, backward, _, _, _, name, map_ptr = _photo_entries(L.load(), ctx.wm)
        L.check(backward(L.ptr(image), L.ptr(target), *map_ptr, C_, H_, W_, lam, weight, L.ptr(go), L.ptr(ws), L.ptr(grad),
                         L.stream_ptr(image.device)), name + "_backward")
        return grad, None, None, None, None


def photometric_loss(image: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2, weight: float = 1.0,
                     return_parts: bool = False, weight_map: Optional[torch.Tensor] = None):
    """The published 3DGS loss `weight * ((1 - lambda) * L1 + lambda * (1 - SSIM))` on [C,H,W] images, fused: one
    tile pass forward (also storing the SSIM derivative maps), one tile pass backward.  `return_parts`: also the
    device tensor [loss, L1, SSIM].
    `weight_map` (EXTENSION, not in the reference, which weights a whole view by the scalar; default None = the loss above): a
    per-pixel weight m, [H,W] or [1,H,W] fp32 on the image's device, one map for all channels, meant to lie in [0,1]:
    `weight * ((1 - lambda) * mean(m |I - G|) + lambda * mean(m (1 - ssim)))` with the published SSIM map - m weights the map's
    VALUE per pixel, it does not enter the window moments - and both means over all C*H*W elements (not divided by sum(m): a
    constant map k is the weight k * weight, a map of ones is the loss without a map).  parts then has FOUR entries
    [loss, mean(m |I - G|), mean(m ssim), mean(m)].  The map is data: no gradient, `requires_grad` is a ValueError."""
    loss, parts = _PhotoLoss.apply(image, target, lambda_dssim, weight, weight_map)
    return (loss, parts) if return_parts else loss


def photometric_loss_step(image: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2, weight: float = 1.0,
                          grad_loss: torch.Tensor = None, weight_map: Optional[torch.Tensor] = None):
    """Value AND image gradient of `photometric_loss` without autograd (`syn3r_photo_loss_step`: the two tile passes, the
    scalar sums formed by the gradient pass' first block instead of a launch of their own).  Returns (loss - a view of
    parts[0] -, parts [loss, L1, SSIM], grad_image); `grad_loss`: device scalar, default 1.  Same bits as
    `_PhotoLoss.forward` + `.backward`.  `weight_map`: as `photometric_loss` (`syn3r_photo_loss_map_step`; parts has 4 entries)."""
    dev, wm = _photo_args("photometric_loss_step", image, target, weight_map)
    image, target = image.detach().contiguous(), target.detach().contiguous()
    lib = L.load()
    C_, H_, W_ = image.shape
    grad = torch.empty_like(image)
    go = grad_loss.to(torch.float32).contiguous() if grad_loss is not None else None
    _, _, step, workspace_bytes, n_parts, name, map_ptr = _photo_entries(lib, wm)
    ws = L.workspace(dev, workspace_bytes(C_, H_, W_), "photo_step")                              # the maps die with the call
    parts = torch.empty(n_parts, dtype=torch.float32, device=dev)
    L.check(step(L.ptr(image), L.ptr(target), *map_ptr, C_, H_, W_, float(lambda_dssim), float(weight), L.ptr(go), L.ptr(parts),
                 L.ptr(grad), L.ptr(ws), ws.numel(), L.stream_ptr(dev)), name + "_step")
    return parts[0], parts, grad


_DCORR_MODES = {"min": 0, "A": 1, "B": 2}      # SYN3R_DCORR_MIN / _A / _B


def _dcorr_args(who: str, depth: torch.Tensor, prior: torch.Tensor, mode: str):
    """(depth, prior) as contiguous fp32 [H*W] views and the mode tag; depth [1,H,W] or [H,W], prior [H,W] or [1,H,W]."""
    L.require_gpu(depth, prior)
    if depth.dtype != torch.float32 or prior.dtype != torch.float32:
        raise ValueError(f"{who}: depth and prior must be float32")
    hw = lambda t: tuple(t.shape[1:]) if t.dim() == 3 and t.shape[0] == 1 else (tuple(t.shape) if t.dim() == 2 else None)
    if hw(depth) is None or hw(prior) is None or hw(depth) != hw(prior):
        raise ValueError(f"{who}: depth [1,H,W] or [H,W] and prior [H,W] or [1,H,W] of the same H, W; got "
                         f"{tuple(depth.shape)} and {tuple(prior.shape)}")
    if mode not in _DCORR_MODES:
        raise ValueError(f"{who}: mode must be one of {sorted(_DCORR_MODES)}, got {mode!r}")
    return depth.detach().contiguous(), prior.detach().contiguous(), _DCORR_MODES[mode]


class _DepthCorrLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth: torch.Tensor, prior: torch.Tensor, weight: float, offset: float, mode: str):
        d, p, m = _dcorr_args("depth_correlation_loss", depth, prior, mode)
        lib = L.load()
        n = d.numel()
        # own buffer, not the shared workspace cache: the statistics must survive until backward
        ws = torch.empty(max(lib.syn3r_depth_corr_loss_workspace_bytes(n), 256), dtype=torch.uint8, device=d.device)
        parts = torch.empty(4, dtype=torch.float32, device=d.device)
        L.check(lib.syn3r_depth_corr_loss(L.ptr(d), L.ptr(p), n, float(weight), float(offset), m, L.ptr(parts), L.ptr(ws),
                                          ws.numel(), L.stream_ptr(d.device)), "depth_corr_loss")
        ctx.save_for_backward(d, p, ws)
        ctx.args = (float(weight), float(offset), m, depth.shape)
        ctx.mark_non_differentiable(parts)
        return parts[0].clone(), parts

    @staticmethod
    def backward(ctx, grad_loss: torch.Tensor, _grad_parts):
        L.join_active_trace()
        d, p, ws = ctx.saved_tensors
        weight, offset, m, shape = ctx.args
        go = grad_loss.to(torch.float32).contiguous()
        grad = torch.empty_like(d)
        L.check(L.load().syn3r_depth_corr_loss_backward(L.ptr(d), L.ptr(p), d.numel(), weight, offset, m, L.ptr(go), L.ptr(ws),
                                                        ws.numel(), L.ptr(grad), L.stream_ptr(d.device)), "depth_corr_loss_backward")
        return grad.reshape(shape), None, None, None, None


def depth_correlation_loss(depth: torch.Tensor, prior: torch.Tensor, weight: float = 1.0, offset: float = 200.0, mode: str = "min",
                           return_parts: bool = False):
    """FSGS' depth-correlation term (Zhu et al., ECCV 2024, "geometry guidance") on one rendered depth map and a monocular prior:
    `weight * min(1 - r_A, 1 - r_B)`, r = Pearson(depth, t) for t = -prior (A) and t = 1 / (prior + offset) (B); `mode` "A" / "B"
    keeps one branch.  The two-branch minimum and offset 200 are recalled from FSGS' train.py (not available): UNPINNED.  A flat
    render or prior gives r = 0 (loss = weight) and a zero gradient, not NaN.  Device scalar, no host synchronisation; backward is
    the kernel's gradient pass through the chosen branch (csrc/depth_loss.hip).  `return_parts`: also the device tensor
    [loss, r_A, r_B, branch (0 = A, 1 = B)]."""
    loss, parts = _DepthCorrLoss.apply(depth, prior, weight, offset, mode)
    return (loss, parts) if return_parts else loss


def depth_correlation_loss_step(depth: torch.Tensor, prior: torch.Tensor, weight: float = 1.0, offset: float = 200.0,
                                mode: str = "min", grad_loss: torch.Tensor = None, return_parts: bool = False):
    """Value AND depth gradient of `depth_correlation_loss` without autograd (`syn3r_depth_corr_loss_step`: two launches).  Returns
    (loss - a view of parts[0] -, grad_depth shaped like depth) [+ parts]; `grad_loss`: device scalar, default 1.  Same bits as
    the autograd Function's forward + backward."""
    d, p, m = _dcorr_args("depth_correlation_loss_step", depth, prior, mode)
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


def _dlocal_args(who: str, depth: torch.Tensor, prior: torch.Tensor, patch: int, origin, mode: str):
    """`_dcorr_args` plus the patch grid: -> (depth, prior, mode tag, (H, W, P, oy, ox)).  The grid's own limits (P in [2, 256], the
    origin in [0, P), at least one full patch) are the library's to reject."""
    d, p, m = _dcorr_args(who, depth, prior, mode)
    try:
        oy, ox = (int(v) for v in origin)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: origin must be a pair (oy, ox) of integers, got {origin!r}") from None
    H, W = (int(v) for v in d.shape[-2:])
    return d, p, m, (H, W, int(patch), oy, ox)


class _DepthCorrLocalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth: torch.Tensor, prior: torch.Tensor, weight: float, patch: int, origin, offset: float, mode: str):
        d, p, m, geom = _dlocal_args("depth_correlation_local_loss", depth, prior, patch, origin, mode)
        lib = L.load()
        # own buffer, not the shared workspace cache: the patch records must survive until backward
        ws = torch.empty(max(lib.syn3r_depth_corr_local_workspace_bytes(*geom), 256), dtype=torch.uint8, device=d.device)
        parts = torch.empty(4, dtype=torch.float32, device=d.device)
        L.check(lib.syn3r_depth_corr_local_loss(L.ptr(d), L.ptr(p), *geom, float(weight), float(offset), m, L.ptr(parts), L.ptr(ws),
                                                ws.numel(), L.stream_ptr(d.device)), "depth_corr_local_loss")
        ctx.save_for_backward(d, p, ws)
        ctx.args = (geom, float(weight), float(offset), m, depth.shape)
        ctx.mark_non_differentiable(parts)
        return parts[0].clone(), parts

    @staticmethod
    def backward(ctx, grad_loss: torch.Tensor, _grad_parts):
        L.join_active_trace()
        d, p, ws = ctx.saved_tensors
        geom, weight, offset, m, shape = ctx.args
        go = grad_loss.to(torch.float32).contiguous()
        grad = torch.empty_like(d)
        L.check(L.load().syn3r_depth_corr_local_loss_backward(L.ptr(d), L.ptr(p), *geom, weight, offset, m, L.ptr(go), L.ptr(ws),
                                                              ws.numel(), L.ptr(grad), 0, L.stream_ptr(d.device)),
                "depth_corr_local_loss_backward")
        return grad.reshape(shape), None, None, None, None, None, None


def depth_correlation_local_loss(depth: torch.Tensor, prior: torch.Tensor, weight: float = 1.0, patch: int = 32, origin=(0, 0),
                                 offset: float = 200.0, mode: str = "min", return_parts: bool = False):
    """The depth-correlation term PATCH-WISE (EXTENSION after SparseGS' patch-based Pearson / DNGaussian's local normalisation: a
    monocular prior is one monotone transform of the depth only locally): `weight / K * sum_k min(1 - r_A, 1 - r_B)` over the K
    `patch` x `patch` tiles of the grid with origin `origin` = (oy, ox), 0 <= oy, ox < patch, that lie inside the image, the
    branch and the flat rule of `depth_correlation_loss` taken per patch; pixels in no full patch have a zero gradient.  The two
    transforms and offset 200 are recalled (UNPINNED).  Device scalar, no host synchronisation; backward is the kernel's gradient pass
    (csrc/depth_loss.hip).  `return_parts`: also the device tensor [loss, mean chosen r, share of patches on B, share of flat patches]."""
    loss, parts = _DepthCorrLocalLoss.apply(depth, prior, weight, patch, origin, offset, mode)
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
    d, p, m, geom = _dlocal_args(who, depth, prior, patch, origin, mode)
    dev = d.device
    lib = L.load()
    if grad_out is not None:
        L.require_gpu(d, grad_out)
        if grad_out.dtype != torch.float32 or grad_out.numel() != d.numel() or not grad_out.is_contiguous():
            raise ValueError(f"{who}: grad_out must be a contiguous float32 tensor of depth's {d.numel()} elements")
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
    d, p, m, geom = _dlocal_args("depth_correlation_local_records", depth, prior, patch, origin, mode)
    lib = L.load()
    H, W, P, oy, ox = geom
    ws = torch.empty(max(lib.syn3r_depth_corr_local_workspace_bytes(*geom), 256), dtype=torch.uint8, device=d.device)
    parts = torch.empty(4, dtype=torch.float32, device=d.device)
    L.check(lib.syn3r_depth_corr_local_loss(L.ptr(d), L.ptr(p), *geom, 1.0, float(offset), m, L.ptr(parts), L.ptr(ws), ws.numel(),
                                            L.stream_ptr(d.device)), "depth_corr_local_loss")
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


def _dsmooth_args(who: str, depth: torch.Tensor, weights: torch.Tensor):
    """(depth, weights) as contiguous fp32 tensors (a view at any 4-byte offset is taken as it is: the library picks its scalar
    path) and (H, W); depth [1,H,W] or [H,W], weights [2,H,W]."""
    L.require_gpu(depth, weights)
    if depth.dtype != torch.float32 or weights.dtype != torch.float32:
        raise ValueError(f"{who}: depth and weights must be float32")
    hw = tuple(depth.shape[1:]) if depth.dim() == 3 and depth.shape[0] == 1 else (tuple(depth.shape) if depth.dim() == 2 else None)
    if hw is None or weights.dim() != 3 or tuple(weights.shape) != (2,) + hw:
        raise ValueError(f"{who}: depth [1,H,W] or [H,W] and weights [2,H,W] of the same H, W; got {tuple(depth.shape)} and "
                         f"{tuple(weights.shape)}")
    return depth.detach().contiguous(), weights.detach().contiguous(), (int(hw[0]), int(hw[1]))


class _DepthSmoothLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth: torch.Tensor, weights: torch.Tensor, weight: float):
        d, w, hw = _dsmooth_args("depth_smoothness_loss", depth, weights)
        lib = L.load()
        # own buffer, not the shared workspace cache: the block rows must survive until backward
        ws = torch.empty(max(lib.syn3r_depth_smooth_workspace_bytes(*hw), 256), dtype=torch.uint8, device=d.device)
        parts = torch.empty(4, dtype=torch.float32, device=d.device)
        L.check(lib.syn3r_depth_smooth_loss(L.ptr(d), L.ptr(w), *hw, float(weight), L.ptr(parts), L.ptr(ws), ws.numel(),
                                            L.stream_ptr(d.device)), "depth_smooth_loss")
        ctx.save_for_backward(d, w, ws)
        ctx.args = (hw, float(weight), depth.shape)
        ctx.mark_non_differentiable(parts)
        return parts[0].clone(), parts

    @staticmethod
    def backward(ctx, grad_loss: torch.Tensor, _grad_parts):
        L.join_active_trace()
        d, w, ws = ctx.saved_tensors
        hw, weight, shape = ctx.args
        go = grad_loss.to(torch.float32).contiguous()
        grad = torch.empty_like(d)
        L.check(L.load().syn3r_depth_smooth_loss_backward(L.ptr(d), L.ptr(w), *hw, weight, L.ptr(go), L.ptr(ws), ws.numel(), L.ptr(grad),
                                                          0, L.stream_ptr(d.device)), "depth_smooth_loss_backward")
        return grad.reshape(shape), None, None


def depth_smoothness_loss(depth: torch.Tensor, weights: torch.Tensor, weight: float = 1.0, return_parts: bool = False):
    """Prior-free edge-aware smoothness of one rendered depth map (EXTENSION; Monodepth2's form): `weight * (S_x + S_y) / m`, m the
    mean depth, S_x the mean over the H (W - 1) horizontal pixel pairs of wx |d[y,x+1] - d[y,x]|, S_y the same over the (H - 1) W
    vertical ones with wy; `weights` = [wx, wy] from `depth_edge_weights` (their last column / row is never read).  The gradient goes
    through the mean; m <= 0 (an empty render) gives 0 and a zero gradient, not NaN.  The division by the mean is recalled from
    Monodepth2: UNPINNED.  Device scalar, no host synchronisation; backward is the kernel's gradient pass (csrc/depth_smooth.hip).
    `return_parts`: also the device tensor [loss, S_x, S_y, m]."""
    loss, parts = _DepthSmoothLoss.apply(depth, weights, weight)
    return (loss, parts) if return_parts else loss


def depth_smoothness_loss_step(depth: torch.Tensor, weights: torch.Tensor, weight: float = 1.0, grad_loss: torch.Tensor = None,
                               grad_out: torch.Tensor = None, return_parts: bool = False):
    """Value AND depth gradient of `depth_smoothness_loss` without autograd (`syn3r_depth_smooth_loss_step`: two launches).  Returns
    (loss - a view of parts[0] -, grad_depth shaped like depth) [+ parts]; `grad_loss`: device scalar, default 1.  `grad_out`
    (float32, contiguous, depth's number of elements, on its device): the gradient is ADDED to it, and it is what comes back;
    without it a new tensor, every pixel written.  Same bits as the autograd Function's forward + backward."""
    who = "depth_smoothness_loss_step"
    d, w, hw = _dsmooth_args(who, depth, weights)
    dev = d.device
    lib = L.load()
    if grad_out is not None:
        L.require_gpu(d, grad_out)
        if grad_out.dtype != torch.float32 or grad_out.numel() != d.numel() or not grad_out.is_contiguous():
            raise ValueError(f"{who}: grad_out must be a contiguous float32 tensor of depth's {d.numel()} elements")
    ws = L.workspace(dev, lib.syn3r_depth_smooth_workspace_bytes(*hw), "dsmooth_step")
    parts = torch.empty(4, dtype=torch.float32, device=dev)
    grad = torch.empty_like(d) if grad_out is None else grad_out
    go = grad_loss.to(torch.float32).contiguous() if grad_loss is not None else None
    L.check(lib.syn3r_depth_smooth_loss_step(L.ptr(d), L.ptr(w), *hw, float(weight), L.ptr(go), L.ptr(parts), L.ptr(grad),
                                             int(grad_out is not None), L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
            "depth_smooth_loss_step")
    return (parts[0], grad, parts) if return_parts else (parts[0], grad)


def _exposure_args(who: str, image: torch.Tensor, A: torch.Tensor, *more: torch.Tensor):
    """The device, and A as a contiguous [12] view: `image` (and every tensor of `more`) float32 [3,H,W] of one shape and contiguous
    (a view at any 4-byte offset is taken as it is: the library picks its scalar path), A float32 with 12 elements."""
    dev = L.require_gpu(image, A, *more)
    if image.dim() != 3 or image.shape[0] != 3 or image.dtype != torch.float32:
        raise ValueError(f"{who}: image must be a float32 [3,H,W] tensor, got {image.dtype} {tuple(image.shape)}")
    if any(t.shape != image.shape or t.dtype != torch.float32 for t in more):
        raise ValueError(f"{who}: every image-shaped argument must be float32 {tuple(image.shape)}")
    if A.dtype != torch.float32 or A.numel() != 12:
        raise ValueError(f"{who}: A must be a float32 tensor of 12 elements (3 x 4, row-major), got {A.dtype} {tuple(A.shape)}")
    return dev, A.detach().contiguous().reshape(12)


def exposure_apply_step(image: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """`E(image)` of a per-camera affine exposure A (3 x 4, row-major, 12 floats on the device) without autograd:
    E_c = A[c][0] I_0 + A[c][1] I_1 + A[c][2] I_2 + A[c][3], no clamp (`syn3r_exposure_apply`, csrc/exposure.hip: one launch)."""
    dev, a = _exposure_args("exposure_apply_step", image, A)
    image = image.detach().contiguous()
    out = torch.empty_like(image)
    L.check(L.load().syn3r_exposure_apply(L.ptr(image), L.ptr(a), int(image.shape[1]), int(image.shape[2]), L.ptr(out), L.stream_ptr(dev)),
            "exposure_apply")
    return out


def exposure_backward_step(image: torch.Tensor, A: torch.Tensor, grad_out: torch.Tensor, grad_A_out: torch.Tensor,
                           accumulate: bool = False) -> torch.Tensor:
    """The backward of `exposure_apply_step` without autograd (`syn3r_exposure_backward`: two launches, no atomics, bitwise
    repeatable): returns grad_image_k = sum_c A[c][k] grad_out_c and STORES grad_A[c][k] = sum_p grad_out_c I_k, grad_A[c][3] =
    sum_p grad_out_c in `grad_A_out` (float32, 12 elements, contiguous, on the device) - or ADDS them to it with `accumulate`."""
    dev, a = _exposure_args("exposure_backward_step", image, A, grad_out)
    L.require_gpu(grad_A_out)
    if grad_A_out.dtype != torch.float32 or grad_A_out.numel() != 12 or not grad_A_out.is_contiguous():
        raise ValueError("exposure_backward_step: grad_A_out must be a contiguous float32 tensor of 12 elements")
    image, grad_out = image.detach().contiguous(), grad_out.detach().contiguous()
    lib = L.load()
    H_, W_ = int(image.shape[1]), int(image.shape[2])
    grad_image = torch.empty_like(image)
    ws = L.workspace(dev, lib.syn3r_exposure_backward_workspace_bytes(H_, W_), "exposure")
    L.check(lib.syn3r_exposure_backward(L.ptr(image), L.ptr(a), L.ptr(grad_out), H_, W_, L.ptr(grad_image), L.ptr(grad_A_out),
                                        int(bool(accumulate)), L.ptr(ws), ws.numel(), L.stream_ptr(dev)), "exposure_backward")
    return grad_image


class _ExposureApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image: torch.Tensor, A: torch.Tensor):
        out = exposure_apply_step(image, A)
        ctx.save_for_backward(image.detach().contiguous(), A.detach())
        return out

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        L.join_active_trace()
        image, A = ctx.saved_tensors
        grad_A = torch.empty(12, dtype=torch.float32, device=image.device)
        grad_image = exposure_backward_step(image, A, grad_out.contiguous(), grad_A)
        return grad_image, grad_A.reshape(A.shape)


def exposure_apply(image: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """`exposure_apply_step` as an autograd operator: its backward is `syn3r_exposure_backward` and returns gradients for both
    `image` and `A` (EXTENSION: the per-camera affine exposure of `OptimizationParams.exposure_opt`)."""
    return _ExposureApply.apply(image, A)


def _mcmc_rows(who: str, n: int, **tensors: torch.Tensor) -> torch.device:
    """The device; every tensor float32 (int32 for the names `src`, `counts`, `weights`), contiguous, with n rows - taken as they
    are (the entries work in place: a copy would be silently dropped)."""
    dev = L.require_gpu(*tensors.values())
    for name, t in tensors.items():
        want = torch.int32 if name in ("src", "counts", "weights") else torch.float32
        if t.dtype != want or not t.is_contiguous() or t.dim() < 1 or (name != "src" and t.shape[0] != n):
            raise ValueError(f"{who}: {name} must be a contiguous {want} tensor with {n} rows, got {t.dtype} {tuple(t.shape)}")
    return dev


def mcmc_noise(xyz: torch.Tensor, log_scales: torch.Tensor, rotations: torch.Tensor, opacity_logits: torch.Tensor, scale: float,
               seed: int, step: int) -> None:
    """3DGS-MCMC's position noise IN PLACE on `xyz` [n,3] (`syn3r_mcmc_noise`, csrc/mcmc.hip: one launch, no host read):
    xyz_i += scale * gate(sigmoid(logit_i)) * Sigma_i eps_i, Sigma_i from the raw log-scales [n,3] and (w, x, y, z) quaternions [n,4],
    gate(o) = 1 / (1 + exp(-100 (0.005 - o))), eps_i the Philox4x32-10 normals of (seed, step, i).  The same (seed, step) gives the
    same bits; recalled constants, UNPINNED (include/syn3r_hip.h)."""
    n = int(xyz.shape[0])
    dev = _mcmc_rows("mcmc_noise", n, xyz=xyz, log_scales=log_scales, rotations=rotations, opacity_logits=opacity_logits)
    if xyz.shape != (n, 3) or log_scales.shape != (n, 3) or rotations.shape != (n, 4) or opacity_logits.numel() != n:
        raise ValueError("mcmc_noise: xyz [n,3], log_scales [n,3], rotations [n,4], opacity_logits [n]")
    L.check(L.load().syn3r_mcmc_noise(L.ptr(xyz), L.ptr(log_scales), L.ptr(rotations), L.ptr(opacity_logits), n, float(scale),
                                      int(seed) & (2 ** 64 - 1), int(step), L.stream_ptr(dev)), "mcmc_noise")


def mcmc_reg_step(opacity_logits: torch.Tensor, log_scales: torch.Tensor, opacity_reg: float, scale_reg: float,
                  grad_opacity: torch.Tensor, grad_log_scales: torch.Tensor) -> torch.Tensor:
    """3DGS-MCMC's two L1 regularisers without autograd (`syn3r_mcmc_reg_step`: two launches, no atomics, bitwise repeatable):
    returns the device tensor [opacity_reg * mean sigmoid(logit), scale_reg * mean exp(log_scale)] and ADDS their gradients with
    respect to the raw parameters to `grad_opacity` [n] and `grad_log_scales` [n,3] in place."""
    n = int(log_scales.shape[0])
    dev = _mcmc_rows("mcmc_reg_step", n, opacity_logits=opacity_logits, log_scales=log_scales, grad_opacity=grad_opacity,
                     grad_log_scales=grad_log_scales)
    if log_scales.shape != (n, 3) or grad_log_scales.shape != (n, 3) or opacity_logits.numel() != n or grad_opacity.numel() != n:
        raise ValueError("mcmc_reg_step: opacity_logits [n], log_scales [n,3] and gradients of the same shapes")
    lib = L.load()
    out = torch.empty(2, dtype=torch.float32, device=dev)
    ws = L.workspace(dev, lib.syn3r_mcmc_reg_step_workspace_bytes(n), "mcmc_reg")
    L.check(lib.syn3r_mcmc_reg_step(L.ptr(opacity_logits), L.ptr(log_scales), n, float(opacity_reg), float(scale_reg),
                                    L.ptr(grad_opacity), L.ptr(grad_log_scales), L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
            "mcmc_reg_step")
    return out


def mcmc_weights(opacity_logits: torch.Tensor, dead_logit: float) -> torch.Tensor:
    """Integer sampling weights [n] int32 (`syn3r_mcmc_weights`): 0 where logit <= dead_logit (dead), else
    rint(sigmoid(logit) * 65536)."""
    n = int(opacity_logits.numel())
    dev = _mcmc_rows("mcmc_weights", opacity_logits.shape[0], opacity_logits=opacity_logits)
    w = torch.empty(n, dtype=torch.int32, device=dev)
    L.check(L.load().syn3r_mcmc_weights(L.ptr(opacity_logits), n, float(dead_logit), L.ptr(w), L.stream_ptr(dev)), "mcmc_weights")
    return w


def mcmc_sample(weights: torch.Tensor, m_extra: int, seed: int, step: int):
    """For every dead row (weight 0) and for `m_extra` rows past the end a live source drawn with probability weight / total
    (`syn3r_mcmc_sample`: integer arithmetic, Philox4x32-10 of (seed, step, destination)): -> (src [n + m_extra] int32, -1 for a live
    row or when every weight is 0; counts [n] int32, how often each row was drawn).  No host read."""
    n = int(weights.numel())
    dev = _mcmc_rows("mcmc_sample", n, weights=weights)
    if weights.dim() != 1 or int(m_extra) < 0:
        raise ValueError("mcmc_sample: weights [n] int32, m_extra >= 0")
    lib = L.load()
    src = torch.empty(n + int(m_extra), dtype=torch.int32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    ws = L.workspace(dev, lib.syn3r_mcmc_sample_workspace_bytes(n), "mcmc_sample")
    L.check(lib.syn3r_mcmc_sample(L.ptr(weights), n, int(m_extra), int(seed) & (2 ** 64 - 1), int(step), L.ptr(src), L.ptr(counts),
                                  L.ptr(ws), ws.numel(), L.stream_ptr(dev)), "mcmc_sample")
    return src, counts


def mcmc_relocate(src: torch.Tensor, counts: torch.Tensor, xyz: torch.Tensor, features: torch.Tensor, opacity_logits: torch.Tensor,
                  log_scales: torch.Tensor, rotations: torch.Tensor, moments, min_opacity: float) -> None:
    """3DGS-MCMC's relocation IN PLACE (`syn3r_mcmc_relocate`: two launches): every source (counts > 0) takes the opacity and scale
    that keep the rendered distribution when counts + 1 Gaussians share its place, every destination d < n with src[d] >= 0 becomes
    a copy of its source with those values.  `moments`: ten tensors or None, (exp_avg, exp_avg_sq) of xyz, features, opacity,
    log_scales, rotations - the rows of every touched Gaussian are zeroed.  `src` may be longer than n (the rows past n are read by
    the caller, who appends them)."""
    import ctypes as C
    n = int(xyz.shape[0])
    moments = list(moments)
    if len(moments) != 10:
        raise ValueError("mcmc_relocate: moments must have ten entries (tensors or None)")
    params = (xyz, features, opacity_logits, log_scales, rotations)
    dev = _mcmc_rows("mcmc_relocate", n, src=src, counts=counts, xyz=xyz, features=features, opacity_logits=opacity_logits,
                     log_scales=log_scales, rotations=rotations)
    if src.numel() < n or xyz.shape != (n, 3) or log_scales.shape != (n, 3) or rotations.shape != (n, 4) or opacity_logits.numel() != n:
        raise ValueError("mcmc_relocate: src [>= n], xyz [n,3], features [n,...], opacity_logits [n], log_scales [n,3], rotations [n,4]")
    for k, m in enumerate(moments):
        if m is not None:
            _mcmc_rows("mcmc_relocate", n, moment=m)
            if m.shape != params[k // 2].shape or m.device != dev:
                raise ValueError(f"mcmc_relocate: moment {k} must have the shape of its parameter, on its device")
    table = (C.c_void_p * 10)(*[None if m is None else m.data_ptr() for m in moments])
    L.check(L.load().syn3r_mcmc_relocate(n, L.ptr(src), L.ptr(counts), L.ptr(xyz), L.ptr(features), int(features[0].numel()),
                                         L.ptr(opacity_logits), L.ptr(log_scales), L.ptr(rotations), table, float(min_opacity),
                                         L.stream_ptr(dev)), "mcmc_relocate")


def image_metrics(image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Device tensor [PSNR (dB, peak 1), SSIM] of two float32 [C,H,W] images in [0,1]: the MSE from `syn3r_image_mse`
    (deterministic two-level sum) and the SSIM the fused photometric-loss kernel computes (published 3DGS window).
    No host synchronisation."""
    L.require_gpu(image, target)
    image, target = image.detach().contiguous(), target.detach().contiguous()
    if image.shape != target.shape or image.dim() != 3 or image.dtype != torch.float32:
        raise ValueError("image_metrics: float32 [C,H,W] images of the same shape")
    lib = L.load()
    n = image.numel()
    mse = torch.empty((), dtype=torch.float32, device=image.device)
    ws = L.workspace(image.device, lib.syn3r_l1_loss_workspace_bytes(n), "l1")
    L.check(lib.syn3r_image_mse(L.ptr(image), L.ptr(target), n, L.ptr(mse), L.ptr(ws), ws.numel(),
                                L.stream_ptr(image.device)), "image_mse")
    _, parts = _PhotoLoss.apply(image, target, 1.0, 1.0, None)
    psnr = -10.0 * torch.log10(mse.clamp_min(1e-12))
    return torch.stack([psnr, parts[2]])


def knn3_mean_dist2(points: torch.Tensor) -> torch.Tensor:
    """Mean squared distance of every point of a [n,3] fp32 cloud (n >= 4) to its three nearest neighbours:
    `distCUDA2` of the simple-knn extension, which FSGS' create_from_pcd turns into the initial Gaussian scales
    (model/diffusionGS.py:1685-1687 -> reset_gaussians_from_pcd).  Exact search on the device (csrc/knn.hip)."""
    L.require_gpu(points)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("knn3_mean_dist2: points must be a float32 [n,3] tensor")
    pts = points.detach().contiguous()
    n = pts.shape[0]
    lib = L.load()
    out = torch.empty(n, dtype=torch.float32, device=pts.device)
    ws = L.workspace(pts.device, lib.syn3r_knn3_workspace_bytes(n), "knn3")
    L.check(lib.syn3r_knn3_mean_dist2(L.ptr(pts), n, L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr(pts.device)), "knn3_mean_dist2")
    return out


def _cloud_arg(who: str, points: torch.Tensor) -> torch.Tensor:
    L.require_gpu(points)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError(f"{who}: points must be a float32 [n,3] tensor")
    return points.detach().contiguous()


def knn3_graph(points: torch.Tensor):
    """The directed 3-nearest-neighbour graph of a [n,3] fp32 cloud (n >= 4): (dist2 [n,3] fp32, index [n,3] int32), per point the
    three other points nearest first, ties broken by the smaller index (`syn3r_knn3_graph`, csrc/knn.hip: the search of
    `knn3_mean_dist2` keeping the indices; `((d0 + d1) + d2) / 3` equals that function's result bit for bit).  The proximity graph
    of FSGS' Gaussian unpooling (`proximity_unpool`)."""
    pts = _cloud_arg("knn3_graph", points)
    n = pts.shape[0]
    lib = L.load()
    dist2 = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    index = torch.empty((n, 3), dtype=torch.int32, device=pts.device)
    ws = L.workspace(pts.device, lib.syn3r_knn3_graph_workspace_bytes(n), "knn3")
    L.check(lib.syn3r_knn3_graph(L.ptr(pts), n, L.ptr(dist2), L.ptr(index), L.ptr(ws), ws.numel(), L.stream_ptr(pts.device)), "knn3_graph")
    return dist2, index


def camera_table(cams) -> torch.Tensor:
    """The [C,16] fp32 HOST table `compute_filter_3D` takes, from FSGS-style cameras (`world_view_transform` = the transposed
    world-to-view matrix, `FoVx` / `FoVy`, `image_width` / `image_height`): per camera the 12 entries of [R | t] row by row, then
    fx, fy, W, H (include/syn3r_hip.h).  One device -> host read per camera: build it when the camera list changes, not per step."""
    import math
    rows = []
    for c in cams:
        w2c = c.world_view_transform.detach().to("cpu", torch.float32).t()
        W, H = float(c.image_width), float(c.image_height)
        fx, fy = W / (2.0 * math.tan(c.FoVx * 0.5)), H / (2.0 * math.tan(c.FoVy * 0.5))
        rows.append(torch.cat([w2c[:3, :].reshape(-1), torch.tensor([fx, fy, W, H], dtype=torch.float32)]))
    return torch.stack(rows) if rows else torch.zeros((0, 16), dtype=torch.float32)


def compute_filter_3D(xyz: torch.Tensor, cam_table: torch.Tensor, variance: float = L.FILTER3D_VARIANCE, near: float = L.FILTER3D_NEAR,
                      margin: float = L.FILTER3D_MARGIN) -> torch.Tensor:
    """Mip-Splatting's 3D smoothing filter size per Gaussian (`syn3r_filter3d_compute`, csrc/filter3d.hip): [N] fp32,
    sqrt(variance) / (max over the cameras that see the Gaussian of fx / z); unseen Gaussians take the largest filter among the
    seen ones, all zero when none is seen.  `xyz` [N,3] and `cam_table` [C,16] (`camera_table`) are fp32 DEVICE tensors.  Two
    launches on the current stream: no host read, no synchronisation.  The constants are RECALLED from the released code: UNPINNED."""
    dev = L.require_gpu(xyz, cam_table)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or cam_table.dim() != 2 or cam_table.shape[1] != 16:
        raise ValueError(f"compute_filter_3D: xyz must be [N,3] and cam_table [C,16], got {tuple(xyz.shape)} and {tuple(cam_table.shape)}")
    pts = xyz.detach().to(torch.float32).contiguous()
    tab = cam_table.detach().to(torch.float32).contiguous()
    n = pts.shape[0]
    lib = L.load()
    out = torch.empty(n, dtype=torch.float32, device=dev)
    ws = L.workspace(dev, lib.syn3r_filter3d_workspace_bytes(n), "filter3d")
    L.check(lib.syn3r_filter3d_compute(L.ptr(pts), n, L.ptr(tab), int(tab.shape[0]), float(variance), float(near), float(margin),
                                       L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr(dev)), "filter3d_compute")
    return out


def proximity_unpool(xyz: torch.Tensor, log_scales: torch.Tensor, opacity_logits: torch.Tensor, confidence: torch.Tensor,
                     score_thresh: float, log_scale_thresh: float) -> dict:
    """FSGS' proximity-guided Gaussian unpooling (Zhu et al., ECCV 2024, section 3.2) on raw parameters: Gaussian i is a source when the
    mean squared distance to its 3 nearest neighbours exceeds `score_thresh` and its largest log-scale exceeds `log_scale_thresh`
    (-inf: off); every source grows one Gaussian at the midpoint of each of its three graph edges, with the DESTINATION's log-scales,
    opacity logit and confidence and the identity rotation; SH coefficients of new Gaussians are zero (the caller's).  Sources in
    ascending index order, neighbours nearest first: bitwise repeatable.  FSGS' source is not available - the score (simple-knn's
    squared quantity), the scale test and the thresholds are UNPINNED, hence arguments.
    Returns {"xyz" [M,3], "scaling" [M,3] (log), "opacity" [M] (logit), "rotation" [M,4], "confidence" [M], "count": M = 3 S,
    "sources": S}.  ONE host read (S) between the count and the emit launches; S = 0 launches no emit."""
    pts = _cloud_arg("proximity_unpool", xyz)
    L.require_gpu(pts, log_scales, opacity_logits, confidence)
    n, dev = pts.shape[0], pts.device
    f32 = lambda t: t.detach().contiguous()
    ls, op, conf = f32(log_scales), f32(opacity_logits).reshape(-1), f32(confidence).reshape(-1)
    if ls.shape != (n, 3) or op.shape != (n,) or conf.shape != (n,) or any(t.dtype != torch.float32 for t in (ls, op, conf)):
        raise ValueError(f"proximity_unpool: float32 log_scales [n,3], opacity_logits [n] and confidence [n] for n={n} points; got "
                         f"{tuple(log_scales.shape)}, {tuple(opacity_logits.shape)}, {tuple(confidence.shape)}")
    lib = L.load()
    dist2, index = knn3_graph(pts)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws = L.workspace(dev, lib.syn3r_gaussian_unpool_workspace_bytes(n), "unpool")
    L.check(lib.syn3r_gaussian_unpool_count(L.ptr(dist2), L.ptr(ls), n, float(score_thresh), float(log_scale_thresh), L.ptr(count),
                                            L.ptr(ws), ws.numel(), L.stream_ptr(dev)), "gaussian_unpool_count")
    S = int(count.item())                                  # the one synchronisation
    M = 3 * S
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = {"xyz": new(M, 3), "scaling": new(M, 3), "opacity": new(M), "rotation": new(M, 4), "confidence": new(M),
           "count": M, "sources": S}
    if S > 0:
        L.check(lib.syn3r_gaussian_unpool_emit(L.ptr(pts), L.ptr(ls), L.ptr(op), L.ptr(conf), L.ptr(index), n, S, M, L.ptr(out["xyz"]),
                                               L.ptr(out["scaling"]), L.ptr(out["opacity"]), L.ptr(out["rotation"]),
                                               L.ptr(out["confidence"]), L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
                "gaussian_unpool_emit")
    return out


class _AdamItem(NamedTuple):
    """One tensor of a `FusedAdam.step` launch table; `row_len` 0: a plain tensor (`lr_tail`, `head_len` unused)."""
    param: torch.Tensor
    grad: torch.Tensor
    state: dict
    lr: float
    eps: float
    lr_tail: float
    row_len: int
    head_len: int


class FusedAdam:
    """`torch.optim.Adam(param_groups, eps=...)` (no weight decay / amsgrad) with one kernel per parameter tensor.
    Keeps torch's `param_groups` / `state` layout so checkpoints and lr schedules written for the torch optimiser
    keep working.
    A group may carry `lr_tail`, `row_len` and `head_len`: its tensors are rows of `row_len` floats whose first `head_len` take
    `lr` and the rest `lr_tail` (`syn3r_adam_step_multi_rows`: the published 3DGS f_dc / f_rest groups as ONE [N, M, 3] tensor
    with row_len = 3 M, head_len = 3).  `row_len` 0 or absent: a plain group."""

    def __init__(self, param_groups: Iterable[dict], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        self.param_groups: List[dict] = []
        for g in param_groups:
            g = dict(g)
            g["params"] = list(g["params"])
            g.setdefault("lr", lr)
            g.setdefault("betas", betas)
            g.setdefault("eps", eps)
            self.param_groups.append(g)
        self.state: dict = {}

    def zero_grad(self, set_to_none: bool = True):
        for g in self.param_groups:
            for p in g["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    @torch.no_grad()
    def step(self):
        """One update of every parameter that has a gradient: ONE launch per (beta1, beta2) and up to 8 tensors
        (`syn3r_adam_step_multi`; the trainer's five / six groups share their betas), element for element `torch.optim.Adam`.
        A chunk with a tensor of a row-split group goes through `syn3r_adam_step_multi_rows` (the plain tensors ride along with
        row_len = 0); a chunk without one takes `syn3r_adam_step_multi` as before."""
        import ctypes as C
        lib = L.load()
        batches: dict = {}
        for g in self.param_groups:
            b1, b2 = g["betas"]
            row_len = int(g.get("row_len") or 0)
            lr_tail, head_len = (float(g["lr_tail"]), int(g["head_len"])) if row_len else (0.0, 0)
            for p in g["params"]:
                if p.grad is None:
                    continue
                L.require_gpu(p)
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError("FusedAdam: parameters must be contiguous float32")
                st = self.state.get(p)
                if st is None:
                    st = self.state[p] = {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
                st["step"] += 1
                grad = p.grad.contiguous()
                batches.setdefault((float(b1), float(b2), p.device), []).append(
                    _AdamItem(p, grad, st, float(g["lr"]), float(g["eps"]), lr_tail, row_len, head_len))
        for (b1, b2, dev), items in batches.items():
            for k0 in range(0, len(items), 8):
                chunk = items[k0:k0 + 8]
                n = len(chunk)
                ptrs = lambda sel: (C.c_void_p * n)(*[sel(it).data_ptr() for it in chunk])
                arr = lambda ctype, sel: (ctype * n)(*[sel(it) for it in chunk])
                tables = (n, ptrs(lambda it: it.param), ptrs(lambda it: it.grad), ptrs(lambda it: it.state["exp_avg"]),
                          ptrs(lambda it: it.state["exp_avg_sq"]), arr(C.c_longlong, lambda it: it.param.numel()),
                          arr(C.c_float, lambda it: it.lr))
                tail = (b1, b2, arr(C.c_float, lambda it: it.eps), arr(C.c_int, lambda it: int(it.state["step"])), L.stream_ptr(dev))
                if any(it.row_len for it in chunk):
                    rc = lib.syn3r_adam_step_multi_rows(*tables, arr(C.c_float, lambda it: it.lr_tail), arr(C.c_int, lambda it: it.row_len),
                                                        arr(C.c_int, lambda it: it.head_len), *tail)
                    L.check(rc, "adam_step_multi_rows")
                else:
                    rc = lib.syn3r_adam_step_multi(*tables, *tail)
                    L.check(rc, "adam_step_multi")
