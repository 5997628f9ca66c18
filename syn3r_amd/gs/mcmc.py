"""3DGS-MCMC density control, host side (EXTENSION: the reference has none, nothing reference-held pins any of this; Kheradmand et al.,
NeurIPS 2024, "3D Gaussian Splatting as Markov Chain Monte Carlo" - every constant is recalled from the paper and its released code,
neither available to check against: UNPINNED).

With `OptimizationParams.mcmc` this control has the seat of `density.DensityControl`: no gradient thresholds, no clone / split / prune,
no opacity reset, no densification statistics.  Every `mcmc_interval` iterations inside (`densify_from_iter`, `mcmc_until_iter`):

  1. relocation: dead Gaussians (opacity <= `mcmc_min_opacity`, decided on the logit) are moved onto live ones drawn with probability
     proportional to opacity; a source that was drawn c times shares its place with c copies, all at the opacity and scale that keep
     what the place renders (`train_ops.mcmc_weights` -> `mcmc_sample` -> `mcmc_relocate`, csrc/mcmc.hip).  In place, no host read.
  2. growth while N < `mcmc_cap_max`: target = min(cap, int(1.05 N)) - host arithmetic on a number the host knows - and target - N
     more draws, whose sources are adjusted the same way and whose copies are appended with zero Adam moments.

Once N == `mcmc_cap_max` a call changes neither N nor any allocation: the rasteriser's binning capacities stay valid.  The random
draws are Philox4x32-10 of (`opt.seed`, the iteration, the destination's index): no generator state, a resumed run continues the
stream.  The per-step noise and the two regularisers are the trainer's (`GSTrainer.train_step`)."""
from __future__ import annotations

import math

import numpy as np
import torch

from .train_ops import mcmc_relocate, mcmc_sample, mcmc_weights

GROWTH = 1.05                             # N grows by 5 % per call until the cap: recalled, UNPINNED


def dead_logit(min_opacity: float) -> float:
    """logit(min_opacity) rounded to fp32: a Gaussian is dead when its fp32 logit is <= this value"""
    return float(np.float32(math.log(min_opacity / (1.0 - min_opacity))))


def clamp_opacity(min_opacity: float) -> float:
    """The lower clamp of a relocated opacity: the smallest fp32 opacity >= `min_opacity` whose logit, as `syn3r_mcmc_relocate`
    forms it (fp64 log of the fp32 clamp, rounded to fp32), lies ABOVE `dead_logit(min_opacity)`.  The released code clamps to the
    threshold itself, where its `<=` test finds the Gaussian dead again at the next call; a few 1e-10 above it a relocated Gaussian
    is alive on arrival - UNPINNED."""
    dead = np.float32(dead_logit(min_opacity))
    c = np.float32(min_opacity)
    while True:
        on = float(c)
        if c >= np.float32(min_opacity) and np.float32(math.log(on / (1.0 - on))) > dead:
            return on
        c = np.nextafter(c, np.float32(1.0))


class MCMCControl:
    """The trainer's side of `OptimizationParams.mcmc`.  It reads the trainer's `gaussians`, `optimizer`, `opt` and `iteration` when
    it needs them, never at construction, and appends through the density control's `_append_gaussians` (the one place that swaps a
    parameter in the model and in its optimiser group)."""

    def __init__(self, trainer):
        self.trainer = trainer
        self.calls = 0                    # control calls that ran (`control`)

    def _moments(self) -> list:
        """(exp_avg, exp_avg_sq) of the five parameter tensors in the optimiser's group order; None for one that has not stepped"""
        tr = self.trainer
        out = []
        for attr in tr.density._PARAM_ATTRS:
            st = tr.optimizer.state.get(getattr(tr.gaussians, attr))
            out += [None, None] if st is None else [st["exp_avg"], st["exp_avg_sq"]]
        return out

    @torch.no_grad()
    def _draw_and_relocate(self, m_extra: int, step: int) -> torch.Tensor:
        """weights -> sample -> relocate on the current set; returns src [N + m_extra] (device, int32)"""
        g, o = self.trainer.gaussians, self.trainer.opt
        w = mcmc_weights(g._opacity.detach(), dead_logit(float(o.mcmc_min_opacity)))
        src, counts = mcmc_sample(w, m_extra, int(o.seed), step)
        mcmc_relocate(src, counts, g._xyz.detach(), g._features.detach(), g._opacity.detach(), g._scaling.detach(), g._rotation.detach(),
                      self._moments(), clamp_opacity(float(o.mcmc_min_opacity)))
        return src

    @torch.no_grad()
    def relocate_and_grow(self, step: int) -> int:
        """One control call: relocation, then growth towards the cap.  Returns the number of Gaussians appended (0 at the cap)."""
        g, o = self.trainer.gaussians, self.trainer.opt
        self._draw_and_relocate(0, step)
        g.filter_3D = None                    # (positions jumped: ensure_filter_3D computes the filter again)
        n = int(g._xyz.shape[0])
        target = min(int(o.mcmc_cap_max), int(GROWTH * n))
        if target <= n:
            return 0
        # (after the relocation no row is dead unless all are: the draws of this call are those of the rows past N, other indices
        # than the first call's, so one step value serves both)
        src = self._draw_and_relocate(target - n, step)
        idx = src[n:].long().clamp_min(0)     # (-1 only when every Gaussian is dead: nothing to copy from, row 0 stands in)
        density = self.trainer.density
        density._append_gaussians({a: getattr(g, a).detach()[idx] for a in density._PARAM_ATTRS}, g.confidence[idx])
        return target - n

    def control(self, out: dict) -> bool:
        """The per-iteration hook (after backward, before the optimiser step).  True when the control ran: the trainer then skips the
        optimiser step, its rule for gradients that belong to the old set, extended to in-place relocation - the paper's loop steps
        first and relocates after: UNPINNED."""
        o, it = self.trainer.opt, self.trainer.iteration + 1
        if not (int(o.densify_from_iter) < it < int(o.mcmc_until_iter)) or it % max(int(o.mcmc_interval), 1) != 0:
            return False
        self.relocate_and_grow(it)
        self.calls += 1
        return True
