"""The operators of 3DGS-MCMC density control on the HIP library (csrc/mcmc.hip): position noise, the two L1 regularisers, and the
weights -> sample -> relocate chain that moves dead Gaussians onto live ones.  All in place or without a host read."""
from __future__ import annotations

import torch

from ... import _lib as L


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
