"""Per-camera affine exposure compensation on the HIP library (csrc/exposure.hip): E(image) of a 3 x 4 matrix and its backward, as
`*_step` functions without autograd and as the autograd operator `exposure_apply`."""
from __future__ import annotations

import torch

from ... import _lib as L


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
