"""The per-camera affine exposure (`syn3r_exposure_apply` / `syn3r_exposure_backward`, include/syn3r_hip.h) restated in float64 torch
on the CPU: `apply`, its backward by closed form (`backward`) and by autograd of `apply` (`backward_autograd`), one Adam step
(`adam_step`, torch.optim.Adam's arithmetic) and the loop the trainer's recovery test sizes its step count with (`recovery`).
A plain module: no fixtures, nothing collected."""
import torch

F64 = torch.float64


def apply(image: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """E_c = A[c][0] I_0 + A[c][1] I_1 + A[c][2] I_2 + A[c][3]; image [3,H,W], A 12 values (3 x 4, row-major)"""
    image, A = image.to(F64), A.to(F64).reshape(3, 4)
    return torch.stack([A[c, 0] * image[0] + A[c, 1] * image[1] + A[c, 2] * image[2] + A[c, 3] for c in range(3)])


def backward(image: torch.Tensor, A: torch.Tensor, grad_out: torch.Tensor):
    """-> (grad_image [3,H,W], grad_A [12]) by closed form"""
    image, A, grad_out = image.to(F64), A.to(F64).reshape(3, 4), grad_out.to(F64)
    grad_image = torch.einsum("ck,chw->khw", A[:, :3], grad_out)
    grad_A = torch.cat([torch.einsum("chw,khw->ck", grad_out, image), grad_out.sum(dim=(1, 2))[:, None]], dim=1)
    return grad_image, grad_A.reshape(12)


def backward_autograd(image: torch.Tensor, A: torch.Tensor, grad_out: torch.Tensor):
    image = image.to(F64).clone().requires_grad_(True)
    A = A.to(F64).reshape(12).clone().requires_grad_(True)
    apply(image, A).backward(grad_out.to(F64))
    return image.grad, A.grad


def grad_A_abs(image: torch.Tensor, grad_out: torch.Tensor) -> torch.Tensor:
    """S_abs [12]: the sums of grad_A with every term replaced by its magnitude"""
    image, grad_out = image.to(F64).abs(), grad_out.to(F64).abs()
    return torch.cat([torch.einsum("chw,khw->ck", grad_out, image), grad_out.sum(dim=(1, 2))[:, None]], dim=1).reshape(12)


def l1(image: torch.Tensor, target: torch.Tensor, weight: float = 1.0):
    """-> (weight * mean |image - target|, its gradient with respect to image)"""
    d = image.to(F64) - target.to(F64)
    return weight * d.abs().mean(), weight * torch.sign(d) / d.numel()


def adam_step(A: torch.Tensor, grad: torch.Tensor, state: dict, lr: float, betas=(0.9, 0.999), eps: float = 1e-15) -> torch.Tensor:
    """One torch.optim.Adam step in float64; `state` = {"m", "v", "t"} is advanced in place, the new A is returned"""
    g = grad.to(F64)
    state["t"] += 1
    state["m"] = betas[0] * state["m"] + (1.0 - betas[0]) * g
    state["v"] = betas[1] * state["v"] + (1.0 - betas[1]) * g * g
    bc1, bc2 = 1.0 - betas[0] ** state["t"], 1.0 - betas[1] ** state["t"]
    return A.to(F64) - (lr / bc1) * state["m"] / (state["v"].sqrt() / bc2 ** 0.5 + eps)


def new_state() -> dict:
    return {"m": torch.zeros(12, dtype=F64), "v": torch.zeros(12, dtype=F64), "t": 0}


IDENTITY = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], dtype=F64)
# the transform the recovery test plants: gains diag(0.8, 0.9, 1.1), every off-diagonal entry 0.05, offsets (0.05, -0.02, 0.03)
A_STAR = torch.tensor([0.8, 0.05, 0.05, 0.05, 0.05, 0.9, 0.05, -0.02, 0.05, 0.05, 1.1, 0.03], dtype=F64)


def recovery(image: torch.Tensor, steps: int, lr: float = 0.01, weight: float = 1.0):
    """Adam on A from the identity against target = apply(image, A_STAR) under plain L1: -> (max|A - A*| per step [steps + 1],
    loss per step [steps + 1]), entry 0 before the first step"""
    image = image.to(F64)
    target = apply(image, A_STAR)
    A, state = IDENTITY.clone(), new_state()
    errs, losses = [], []
    for _ in range(steps + 1):
        loss, d = l1(apply(image, A), target, weight)
        errs.append(float((A - A_STAR).abs().max()))
        losses.append(float(loss))
        A = adam_step(A, backward(image, A, d)[1], state, lr)
    return errs, losses
