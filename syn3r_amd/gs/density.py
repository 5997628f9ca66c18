"""Adaptive density control of the trainer.

FSGS' training loop (un-vendored) densifies with the published 3DGS clone / split / prune rules plus its own
proximity-guided unpooling; the published rules are restated here (Kerbl et al. 2023 section 5.2, UNPINNED: checked
against oracle/densify_oracle.py); the FSGS-specific unpooling follows the paper's section 3.2 (`proximity_unpool`, no source:
its constants are options).  Everything runs on the device; the optimiser moments follow the Gaussians."""
from __future__ import annotations

import math
from typing import Optional

import torch

from .gaussian_model import build_rotation
from .train_ops import proximity_unpool as _proximity_unpool_op


class DensityControl:
    """Owns every change of the SET of Gaussians during training.  It reads the trainer's `gaussians`, `optimizer`, `opt`,
    `iteration` and `cameras_extent()` when it needs them (the orchestrator replaces the optimiser and may replace `opt`), so it
    holds the trainer, the seeded generator of the split noise and `last_unpooled`.  Where one of its public operations runs another
    (`control` -> `densify_and_prune` / `reset_opacity`, `densify_and_prune` -> `proximity_unpool`) it calls the trainer's method
    of that name: those are the seams tests and tools replace on the trainer instance."""

    _PARAM_ATTRS = ("_xyz", "_features", "_opacity", "_scaling", "_rotation")     # = order of the optimiser groups

    def __init__(self, trainer):
        self.trainer = trainer
        self.last_unpooled = 0            # Gaussians the proximity unpooling added in the last densify_and_prune call
        self._noise_gen = torch.Generator(device=trainer.gaussians._xyz.device)
        self._noise_gen.manual_seed(int(trainer.opt.seed) + 12345)

    def _swap_param(self, attr: str, tensor: torch.Tensor, moments=None):
        """Replace parameter `attr` by `tensor` in the model and in its optimiser group; `moments` maps the old
        (exp_avg, exp_avg_sq) to the new ones (None: start from zero, as a fresh parameter)."""
        g, optimizer = self.trainer.gaussians, self.trainer.optimizer
        old = getattr(g, attr)
        new = torch.nn.Parameter(tensor.contiguous())
        grp = optimizer.param_groups[self._PARAM_ATTRS.index(attr)]
        st = optimizer.state.pop(old, None)
        if st is not None and moments is not None:
            st["exp_avg"], st["exp_avg_sq"] = moments(st["exp_avg"]).contiguous(), moments(st["exp_avg_sq"]).contiguous()
            optimizer.state[new] = st
        grp["params"] = [new]
        setattr(g, attr, new)

    @torch.no_grad()
    def _append_gaussians(self, ext: dict, confidence: torch.Tensor):
        g = self.trainer.gaussians
        for attr in self._PARAM_ATTRS:
            e = ext[attr]
            self._swap_param(attr, torch.cat([getattr(g, attr).detach(), e]),
                             moments=lambda m, e=e: torch.cat([m, torch.zeros_like(e)]))
        g.confidence = torch.cat([g.confidence, confidence])
        g.filter_3D = None                    # (ensure_filter_3D: a prune after a clone may give the old N back)
        g.xyz_gradient_accum = None           # statistics restart after every change of the set (published postfix)
        g.ensure_stats()

    @torch.no_grad()
    def _keep_gaussians(self, keep: torch.Tensor):
        g = self.trainer.gaussians
        g.ensure_stats()
        for attr in self._PARAM_ATTRS:
            self._swap_param(attr, getattr(g, attr).detach()[keep], moments=lambda m: m[keep])
        g.confidence = g.confidence[keep]
        g.filter_3D = None
        acc_abs = g.xyz_gradient_accum_abs
        g.xyz_gradient_accum, g.denom, g.max_radii2D = g.xyz_gradient_accum[keep], g.denom[keep], g.max_radii2D[keep]
        g.xyz_gradient_accum_abs = acc_abs[keep] if acc_abs is not None else None

    def _split_noise(self, n: int) -> torch.Tensor:
        """Standard-normal draws [n,3] for the split positions (seeded per trainer: runs are reproducible)."""
        return torch.randn((n, 3), generator=self._noise_gen, device=self.trainer.gaussians._xyz.device)

    @torch.no_grad()
    def proximity_unpool(self, extent: float) -> int:
        """FSGS' proximity-guided unpooling (Zhu et al., ECCV 2024, section 3.2) on the current model: the HIP operator
        `train_ops.proximity_unpool` with score_thresh = proximity_dist_factor x extent and log_scale_thresh =
        log(proximity_scale_factor x extent), the new Gaussians appended with zero SH coefficients and zero Adam moments; the
        densification statistics restart.  Returns the number appended (3 per source); fewer than 4 Gaussians or no source: 0 and
        nothing is touched.  One host synchronisation (the source count)."""
        g, o = self.trainer.gaussians, self.trainer.opt
        if g._xyz.shape[0] < 4:
            return 0
        scale = float(o.proximity_scale_factor) * float(extent)
        new = _proximity_unpool_op(g._xyz, g._scaling, g._opacity, g.confidence, float(o.proximity_dist_factor) * float(extent),
                                   math.log(scale) if scale > 0.0 else -math.inf)
        m = int(new["count"])
        if m == 0:
            return 0
        feats = torch.zeros((m,) + tuple(g._features.shape[1:]), dtype=g._features.dtype, device=g._features.device)
        self._append_gaussians({"_xyz": new["xyz"], "_features": feats, "_opacity": new["opacity"].reshape((m,) + tuple(g._opacity.shape[1:])),
                                "_scaling": new["scaling"], "_rotation": new["rotation"]}, new["confidence"])
        return m

    @torch.no_grad()
    def densify_and_prune(self, max_grad: float, min_opacity: float, extent: float, max_screen_size: Optional[float]):
        """Published 3DGS `densify_and_prune`: clone small Gaussians with a large view-space gradient, split large ones
        into two (positions sampled from the Gaussian, scales / 1.6), then prune transparent, screen-filling and
        world-huge ones.  Returns (cloned, split, pruned).  With `opt.use_proximity_densify`, before `opt.proximity_until_iter`,
        FSGS' `proximity_unpool` runs between the split and the prune; what it added is `self.last_unpooled`.
        With `opt.densify_abs_grad` the split is AbsGS' rule: large Gaussians whose accumulated ABSOLUTE gradient
        (`xyz_gradient_accum_abs / denom`) reaches `opt.densify_abs_grad_threshold`; the clone keeps the plain gradient and `max_grad`."""
        g, o = self.trainer.gaussians, self.trainer.opt
        self.last_unpooled = 0
        g.ensure_stats(bool(o.densify_abs_grad))
        grads = g.xyz_gradient_accum / g.denom
        grads[grads.isnan()] = 0.0
        split_grads, split_thresh = grads, max_grad
        if o.densify_abs_grad:
            split_grads = g.xyz_gradient_accum_abs / g.denom
            split_grads[split_grads.isnan()] = 0.0
            split_thresh = float(o.densify_abs_grad_threshold)
        max_radii = g.max_radii2D.clone()
        # ---- clone
        sel = (torch.norm(grads, dim=-1) >= max_grad) & (g.get_scaling.max(dim=1).values <= o.percent_dense * extent)
        n_clone = int(sel.sum())
        self._append_gaussians({a: getattr(g, a).detach()[sel] for a in self._PARAM_ATTRS}, g.confidence[sel])
        max_radii = torch.cat([max_radii, torch.zeros(n_clone, device=max_radii.device)])
        # ---- split (the clones carry a zero gradient)
        n_now = g._xyz.shape[0]
        padded = torch.zeros(n_now, device=g._xyz.device)
        padded[:split_grads.shape[0]] = split_grads.squeeze(-1)
        sel = (padded >= split_thresh) & (g.get_scaling.max(dim=1).values > o.percent_dense * extent)
        n_split = int(sel.sum())
        N = 2
        stds = g.get_scaling[sel].repeat(N, 1)
        samples = self._split_noise(N * n_split) * stds
        rots = build_rotation(g._rotation.detach()[sel]).repeat(N, 1, 1)
        ext = {"_xyz": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + g._xyz.detach()[sel].repeat(N, 1),
               "_scaling": torch.log(g.get_scaling[sel].repeat(N, 1) / (0.8 * N)),
               "_rotation": g._rotation.detach()[sel].repeat(N, 1),
               "_features": g._features.detach()[sel].repeat(N, 1, 1),
               "_opacity": g._opacity.detach()[sel].repeat(N)}
        self._append_gaussians(ext, g.confidence[sel].repeat(N))
        max_radii = torch.cat([max_radii, torch.zeros(N * n_split, device=max_radii.device)])
        keep = ~torch.cat([sel, torch.zeros(N * n_split, dtype=torch.bool, device=sel.device)])
        self._keep_gaussians(keep)
        max_radii = max_radii[keep]
        # ---- FSGS' proximity-guided unpooling (recalled order of its densification: clone, split, proximity, prune)
        if o.use_proximity_densify and self.trainer.iteration + 1 < o.proximity_until_iter:
            self.last_unpooled = self.trainer.proximity_unpool(extent)
            max_radii = torch.cat([max_radii, torch.zeros(self.last_unpooled, device=max_radii.device)])
        # ---- prune
        prune = g.get_opacity < min_opacity
        if max_screen_size:
            prune = prune | (max_radii > max_screen_size) | (g.get_scaling.max(dim=1).values > 0.1 * extent)
        n_prune = int(prune.sum())
        self._keep_gaussians(~prune)
        g.xyz_gradient_accum = None
        g.ensure_stats()
        return n_clone, n_split, n_prune

    @torch.no_grad()
    def reset_opacity(self):
        """Published `reset_opacity`: opacity <- min(opacity, 0.01), Adam moments of the opacity restart."""
        g = self.trainer.gaussians
        o = torch.min(g.get_opacity, torch.full_like(g.get_opacity, 0.01))
        self._swap_param("_opacity", torch.log(o / (1 - o)), moments=lambda m: torch.zeros_like(m))

    def control(self, out: dict):
        """The per-iteration hook of the published training loop (after backward, before the optimiser step); `out` is what either
        step route of the trainer returns."""
        g, o, it = self.trainer.gaussians, self.trainer.opt, self.trainer.iteration + 1
        if it >= o.densify_until_iter:
            return
        vis = out["visibility_filter"]
        vgrad = out["viewspace_grad"] if "viewspace_grad" in out else out["viewspace_points"].grad
        g.add_densification_stats(vgrad, vis, out["radii"], abs_grad=out.get("viewspace_abs_grad") if o.densify_abs_grad else None)
        if it > o.densify_from_iter and it % o.densification_interval == 0:
            size = o.prune_screen_size if it > o.opacity_reset_interval else None
            self.trainer.densify_and_prune(o.densify_grad_threshold, o.prune_min_opacity, self.trainer.cameras_extent(), size)
        if it % o.opacity_reset_interval == 0:
            self.trainer.reset_opacity()
