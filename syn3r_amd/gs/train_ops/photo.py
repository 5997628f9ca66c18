"""The image losses of the trainer on the HIP library (csrc/train.hip, csrc/photo_loss.hip): the L1 loss and the published 3DGS
photometric loss (L1 + D-SSIM), each as an autograd operator and as a `*_step` function without autograd, both with an optional
per-pixel weight map, and `image_metrics` (PSNR, SSIM)."""
from __future__ import annotations

from typing import Optional

import torch

from ... import _lib as L


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
