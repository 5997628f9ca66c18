"""The multi-view photometric reprojection term of the trainer on the HIP library (csrc/reproj.hip; the formulas are in
include/syn3r_hip.h): an autograd operator with gradients for the rendered depth AND alpha, a `*_step` function without autograd, and
the per-pixel records for diagnostics.  The host side (relative views, source rule, cache) is `gs/reproj.py`."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ... import _lib as L
from .depth import _check_grad_out, _hw

_ROW_BYTES = 1024 * 16          # head of the workspace (kRpRowBytes of csrc/reproj.hip); the dL/dz and record planes follow


def _inputs(who: str, depth, alpha, target, sources, views):
    """-> (depth, alpha, target as contiguous fp32 tensors (a view at any 4-byte offset is taken as it is: the library picks its
    scalar path), the source tensors, the table of their pointers, the two fp32 host tables, (H, W, S))"""
    sources = list(sources)
    L.require_gpu(depth, alpha, target, *sources)
    hw = _hw(depth)
    if hw is None or _hw(alpha) != hw or depth.dtype != torch.float32 or alpha.dtype != torch.float32:
        raise ValueError(f"{who}: depth and alpha must be float32 [1,H,W] or [H,W] of the same H, W; got {depth.dtype} "
                         f"{tuple(depth.shape)} and {alpha.dtype} {tuple(alpha.shape)}")
    images = [target] + sources
    if any(t.dtype != torch.float32 or tuple(t.shape) != (3,) + hw for t in images):
        raise ValueError(f"{who}: target and every source must be float32 [3,H,W] of depth's H, W = {hw}; got "
                         f"{[tuple(t.shape) for t in images]}")
    try:
        target_k, table = views
        target_k = np.ascontiguousarray(np.asarray(target_k, dtype=np.float32).reshape(-1))
        table = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
    except (TypeError, ValueError):
        raise ValueError(f"{who}: views must be a pair (target_k [4], table [S,16]) (gs.reproj.ReprojViews)") from None
    S = len(sources)
    if target_k.shape != (4,) or table.shape != (S, 16):
        raise ValueError(f"{who}: views must be (target_k [4], table [S,16]) for the S = {S} sources; got {target_k.shape} and {table.shape}")
    srcs = [s.detach().contiguous() for s in sources]
    ptrs = (C.c_void_p * max(S, 1))(*[s.data_ptr() for s in srcs])
    return (depth.detach().contiguous(), alpha.detach().contiguous(), target.detach().contiguous(), srcs, ptrs,
            target_k.ctypes.data_as(C.c_void_p), table.ctypes.data_as(C.c_void_p), (target_k, table), (int(hw[0]), int(hw[1]), S))


def _forward(d, a, t, ptrs, tk, tab, geom, weight: float, alpha_min: float):
    """`syn3r_photo_reproj_loss`: -> (parts [4], the workspace it filled)"""
    lib = L.load()
    # own buffer, not the shared workspace cache: what the statistics pass leaves must survive until backward
    ws = torch.empty(max(lib.syn3r_photo_reproj_workspace_bytes(*geom), 256), dtype=torch.uint8, device=d.device)
    parts = torch.empty(4, dtype=torch.float32, device=d.device)
    L.check(lib.syn3r_photo_reproj_loss(L.ptr(d), L.ptr(a), L.ptr(t), ptrs, tab, tk, *geom, float(weight), float(alpha_min), L.ptr(parts),
                                        L.ptr(ws), ws.numel(), L.stream_ptr(d.device)), "photo_reproj_loss")
    return parts, ws


class _PhotoReprojection(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, target, sources, views, weight, alpha_min):
        d, a, t, srcs, ptrs, tk, tab, keep, geom = _inputs("photo_reprojection_loss", depth, alpha, target, sources, views)
        parts, ws = _forward(d, a, t, ptrs, tk, tab, geom, weight, alpha_min)
        ctx.save_for_backward(d, a, ws)
        ctx.args = (geom, float(weight), float(alpha_min), depth.shape, alpha.shape)
        ctx.mark_non_differentiable(parts)
        return parts[0].clone(), parts

    @staticmethod
    def backward(ctx, grad_loss, _grad_parts):
        L.join_active_trace()
        d, a, ws = ctx.saved_tensors
        geom, weight, alpha_min, d_shape, a_shape = ctx.args
        go = grad_loss.to(torch.float32).contiguous()
        g_depth, g_alpha = torch.empty_like(d), torch.empty_like(a)
        L.check(L.load().syn3r_photo_reproj_loss_backward(L.ptr(d), L.ptr(a), *geom, weight, alpha_min, L.ptr(go), L.ptr(ws), ws.numel(),
                                                          L.ptr(g_depth), 0, L.ptr(g_alpha), 0, L.stream_ptr(d.device)),
                "photo_reproj_loss_backward")
        return g_depth.reshape(d_shape), g_alpha.reshape(a_shape), None, None, None, None, None


def photo_reprojection_loss(depth: torch.Tensor, alpha: torch.Tensor, target: torch.Tensor, sources, views, weight: float = 1.0,
                            alpha_min: float = 0.5, return_parts: bool = False):
    """Multi-view photometric reprojection term (EXTENSION; Monodepth2's per-pixel minimum reprojection error without its SSIM part
    and auto-mask): the rendered `depth` and `alpha` ([1,H,W] or [H,W]) of a target view carry each pixel, at the depth along its ray
    z = depth / alpha, into the `sources` (1 to 4 photographs [3,H,W] of posed input views); `weight` x the mean over the live
    pixels of e = min over the valid sources of (1/3) sum_c |I_s,c(q) - target_c(p)|, bilinear.  A pixel is dead (no loss, zero
    gradients) when alpha < `alpha_min`, depth <= 0 or no source sees it; no live pixel gives 0, not NaN.  `views`:
    `gs.reproj.ReprojViews` (target intrinsics and per source the relative pose and intrinsics, fp32, from float64 on the host).
    Gradients for depth AND alpha, through the chosen source only, the live count held constant (csrc/reproj.hip).  The minimum and
    the L1 form are recalled from Monodepth2; alpha_min = 0.5, no SSIM and no auto-mask are this project's choices: UNPINNED.  Device
    scalar, no host synchronisation.  `return_parts`: also the device tensor [loss, mean e over live pixels, N_live / (H W), share
    of live pixels on source 0]."""
    loss, parts = _PhotoReprojection.apply(depth, alpha, target, tuple(sources), views, weight, alpha_min)
    return (loss, parts) if return_parts else loss


def photo_reprojection_loss_step(depth: torch.Tensor, alpha: torch.Tensor, target: torch.Tensor, sources, views, weight: float = 1.0,
                                 alpha_min: float = 0.5, grad_loss: torch.Tensor = None, grad_out: torch.Tensor = None,
                                 grad_alpha_out: torch.Tensor = None, return_parts: bool = False):
    """Value AND both gradients of `photo_reprojection_loss` without autograd (`syn3r_photo_reproj_loss_step`: two launches).
    Returns (loss - a view of parts[0] -, g_depth shaped like depth, g_alpha shaped like alpha) [+ parts]; `grad_loss`: device scalar,
    default 1.  `grad_out` / `grad_alpha_out` (float32, contiguous, depth's number of elements, on its device): the gradient is
    ADDED to it, and it is what comes back; without it a new tensor, every pixel written (dead pixels 0).  Same bits as the autograd
    Function's forward + backward."""
    who = "photo_reprojection_loss_step"
    d, a, t, srcs, ptrs, tk, tab, keep, geom = _inputs(who, depth, alpha, target, sources, views)
    dev = d.device
    lib = L.load()
    for name, out in (("grad_out", grad_out), ("grad_alpha_out", grad_alpha_out)):
        if out is not None:
            _check_grad_out(who, d, out, name)
    ws = L.workspace(dev, lib.syn3r_photo_reproj_workspace_bytes(*geom), "photo_reproj_step")
    parts = torch.empty(4, dtype=torch.float32, device=dev)
    g_depth = torch.empty_like(d) if grad_out is None else grad_out
    g_alpha = torch.empty_like(a) if grad_alpha_out is None else grad_alpha_out
    go = grad_loss.to(torch.float32).contiguous() if grad_loss is not None else None
    L.check(lib.syn3r_photo_reproj_loss_step(L.ptr(d), L.ptr(a), L.ptr(t), ptrs, tab, tk, *geom, float(weight), float(alpha_min), L.ptr(go),
                                             L.ptr(parts), L.ptr(g_depth), int(grad_out is not None), L.ptr(g_alpha),
                                             int(grad_alpha_out is not None), L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
            "photo_reproj_loss_step")
    return (parts[0], g_depth, g_alpha, parts) if return_parts else (parts[0], g_depth, g_alpha)


def photo_reprojection_records(depth: torch.Tensor, alpha: torch.Tensor, target: torch.Tensor, sources, views, alpha_min: float = 0.5):
    """Per pixel what the statistics pass decided (diagnostics and tests): (e [H,W] fp32, source [H,W] int32, -1 = dead).  e is the
    record word of the workspace: the kernel's fp32 e with its two lowest mantissa bits cleared (they carry the source), 0 for a
    dead pixel."""
    d, a, t, srcs, ptrs, tk, tab, keep, geom = _inputs("photo_reprojection_records", depth, alpha, target, sources, views)
    _, ws = _forward(d, a, t, ptrs, tk, tab, geom, 1.0, alpha_min)
    H, W, _ = geom
    rec = ws[_ROW_BYTES + 4 * H * W:_ROW_BYTES + 8 * H * W].view(torch.int32).reshape(H, W)
    dead = rec == -1
    source = torch.where(dead, rec, rec & 3)
    e = torch.where(dead, torch.zeros_like(rec), rec & ~3).view(torch.float32)
    return e.clone(), source
