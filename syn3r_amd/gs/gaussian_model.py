"""The trainable Gaussians of the trainer (`gs/trainer.py`): parameters with the published activations, the densification statistics,
checkpoint capture / restore and the initialisation from a point cloud."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from .. import _lib as L
from .train_ops import knn3_mean_dist2

SH_C0 = 0.28209479177387814


def build_rotation(q: torch.Tensor) -> torch.Tensor:
    """Rotation matrices [n,3,3] of (w, x, y, z) quaternions, normalised first (published 3DGS general_utils)."""
    q = q / torch.norm(q, dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.empty((q.shape[0], 3, 3), dtype=q.dtype, device=q.device)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - r * z); R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y); R[:, 2, 1] = 2 * (y * z + r * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


class GaussianModel:
    """Trainable Gaussian parameters with the published activations (exp scale, sigmoid opacity, unit quaternion).
    `active_sh_degree` (None: `sh_degree`): the degree the rasteriser evaluates; the published training starts at 0 and raises
    it with `oneupSHdegree` (`OptimizationParams.sh_degree_interval`)."""

    def __init__(self, xyz, log_scales, rotations, opacity_logits, shs, sh_degree: int = 3, device="cuda",
                 active_sh_degree: Optional[int] = None):
        dev = torch.device(device)
        p = lambda t: torch.nn.Parameter(torch.as_tensor(t, dtype=torch.float32).to(dev).contiguous())
        self._xyz, self._scaling, self._rotation = p(xyz), p(log_scales), p(rotations)
        self._opacity, self._features = p(opacity_logits), p(shs)
        self.confidence = torch.ones(self._xyz.shape[0], device=dev)
        # Mip-Splatting's 3D smoothing filter: None, or one filter size per Gaussian ([N] fp32, `train_ops.compute_filter_3D`; kept
        # by `GSTrainer.ensure_filter_3D` when `OptimizationParams.filter_3d` is on).  Data, not a parameter.
        self.filter_3D: Optional[torch.Tensor] = None
        # densification statistics: None until `ensure_stats` makes them for the current set of Gaussians
        self.xyz_gradient_accum = self.denom = self.max_radii2D = self.xyz_gradient_accum_abs = None
        self.max_sh_degree = sh_degree
        self.active_sh_degree = sh_degree if active_sh_degree is None else int(active_sh_degree)
        if not 0 <= self.active_sh_degree <= self.max_sh_degree:
            raise ValueError(f"GaussianModel: active_sh_degree={active_sh_degree} must be in 0..sh_degree={sh_degree}")

    def parameters(self):
        return [self._xyz, self._features, self._opacity, self._scaling, self._rotation]

    def oneupSHdegree(self):
        """Published `GaussianModel.oneupSHdegree`: one more active SH band, up to `max_sh_degree`.  The kernels take any
        sh_degree <= sqrt(coefficients) - 1 and write exact zeros to the gradient of the inactive rows."""
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    @property
    def get_xyz(self): return self._xyz
    @property
    def get_scaling(self): return torch.exp(self._scaling)
    @property
    def get_rotation(self): return torch.nn.functional.normalize(self._rotation)
    @property
    def get_opacity(self): return torch.sigmoid(self._opacity)
    @property
    def get_features(self): return self._features

    # ---- densification statistics (published 3DGS GaussianModel: xyz_gradient_accum / denom / max_radii2D)
    def ensure_stats(self, abs_grad: bool = False):
        """`abs_grad`: also keep `xyz_gradient_accum_abs`, the accumulator of AbsGS' absolute screen-space gradient
        (`OptimizationParams.densify_abs_grad`); it restarts with the other statistics."""
        n, dev = self._xyz.shape[0], self._xyz.device
        if self.xyz_gradient_accum is None or self.xyz_gradient_accum.shape[0] != n:
            self.xyz_gradient_accum = torch.zeros(n, 1, device=dev)
            self.denom = torch.zeros(n, 1, device=dev)
            self.max_radii2D = torch.zeros(n, device=dev)
            self.xyz_gradient_accum_abs = None
        if abs_grad and (self.xyz_gradient_accum_abs is None or self.xyz_gradient_accum_abs.shape[0] != n):
            self.xyz_gradient_accum_abs = torch.zeros(n, 1, device=dev)

    @torch.no_grad()
    def add_densification_stats(self, viewspace_grad: torch.Tensor, update_filter: torch.Tensor, radii: Optional[torch.Tensor] = None,
                                abs_grad: Optional[torch.Tensor] = None):
        """Accumulate the norm of the screen-space positional gradient of the visible Gaussians (3DGS section 5.2: the
        quantity the clone / split decision thresholds) and their largest screen radius.  `abs_grad` ([N,2], the rasteriser's
        absolute screen-space gradient): its norm goes into `xyz_gradient_accum_abs` for the same Gaussians (AbsGS section 3.2)."""
        self.ensure_stats(abs_grad is not None)
        if (radii is not None and update_filter is None and viewspace_grad.is_cuda and viewspace_grad.dtype == torch.float32
                and viewspace_grad.is_contiguous() and radii.dtype == torch.int32
                and (abs_grad is None or (abs_grad.is_cuda and abs_grad.dtype == torch.float32 and abs_grad.is_contiguous()))):
            # the training loop's case (visible = radii > 0): one HIP launch, no boolean-mask indexing (each of which is a
            # `nonzero` with a device -> host synchronisation)
            if abs_grad is not None:
                L.check(L.load().syn3r_densification_stats_abs(int(radii.shape[0]), L.ptr(radii), L.ptr(viewspace_grad), L.ptr(abs_grad),
                                                               L.ptr(self.xyz_gradient_accum), L.ptr(self.xyz_gradient_accum_abs),
                                                               L.ptr(self.denom), L.ptr(self.max_radii2D),
                                                               L.stream_ptr(viewspace_grad.device)), "densification_stats_abs")
                return
            L.check(L.load().syn3r_densification_stats(int(radii.shape[0]), L.ptr(radii), L.ptr(viewspace_grad),
                                                       L.ptr(self.xyz_gradient_accum), L.ptr(self.denom), L.ptr(self.max_radii2D),
                                                       L.stream_ptr(viewspace_grad.device)), "densification_stats")
            return
        if update_filter is None:
            update_filter = radii > 0
        self.xyz_gradient_accum[update_filter] += torch.norm(viewspace_grad[update_filter, :2], dim=-1, keepdim=True)
        if abs_grad is not None:
            self.xyz_gradient_accum_abs[update_filter] += torch.norm(abs_grad[update_filter, :2], dim=-1, keepdim=True)
        self.denom[update_filter] += 1
        if radii is not None:
            self.max_radii2D[update_filter] = torch.max(self.max_radii2D[update_filter], radii[update_filter].to(self.max_radii2D.dtype))

    def capture(self) -> dict:
        """Parameter tensors of a checkpoint (published 3DGS `GaussianModel.capture`, reduced to what this model holds).
        `filter_3D` is added only when the model has one: a checkpoint written with the option off has the keys it always had."""
        state = dict(active_sh_degree=self.active_sh_degree, xyz=self._xyz.detach().clone(),
                     features=self._features.detach().clone(), scaling=self._scaling.detach().clone(),
                     rotation=self._rotation.detach().clone(), opacity=self._opacity.detach().clone(),
                     confidence=self.confidence.clone())
        if self.filter_3D is not None:
            state["filter_3D"] = self.filter_3D.detach().clone()
        return state

    def restore(self, state: dict):
        dev = self._xyz.device
        p = lambda t: torch.nn.Parameter(t.to(dev, torch.float32).contiguous())
        self._xyz, self._features, self._scaling = p(state["xyz"]), p(state["features"]), p(state["scaling"])
        self._rotation, self._opacity = p(state["rotation"]), p(state["opacity"])
        self.confidence = state["confidence"].to(dev)
        self.active_sh_degree = int(state["active_sh_degree"])
        f3 = state.get("filter_3D")
        self.filter_3D = f3.to(dev, torch.float32).contiguous() if f3 is not None else None

    def set_from_pcd(self, points: np.ndarray, colors: np.ndarray, append: bool):
        """Published 3DGS `create_from_pcd`: DC colour = (rgb - 0.5) / C0, higher SH zero, isotropic scale =
        sqrt(mean squared distance to the 3 nearest neighbours), identity rotation, opacity 0.1.  The reference does this
        inside FSGS (`simple-knn` CUDA extension, absent); the exact 3-NN search is `csrc/knn.hip` (`train_ops.knn3_mean_dist2`).
        `active_sh_degree` is left alone (the published `create_from_pcd` runs on a fresh model at degree 0; whether FSGS' fork
        restarts the degree when the orchestrator re-initialises from a point cloud is not visible - UNPINNED)."""
        dev = self._xyz.device
        to_dev = lambda a: (a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).to(dev, torch.float32)
        pts, rgb = to_dev(points), to_dev(colors)
        if pts.dim() != 2 or pts.shape[1] != 3 or rgb.shape != pts.shape:
            raise ValueError("reset_gaussians_from_pcd: points and colours must both be [n,3]")
        n = pts.shape[0]
        if n >= 4:
            d2 = knn3_mean_dist2(pts)                 # HIP: exact 3-NN (csrc/knn.hip), the simple-knn quantity
        else:                                         # degenerate clouds (fewer than 3 neighbours): mean over what there is
            d = torch.cdist(pts, pts) ** 2
            d2 = d.topk(n, dim=1, largest=False).values[:, 1:].mean(1) if n > 1 else torch.full((n,), 1e-4, device=dev)
        scales = torch.log(torch.sqrt(d2.clamp_min(1e-7)))[:, None].repeat(1, 3)
        M = self._features.shape[1]
        feats = torch.zeros(n, M, 3, device=dev)
        feats[:, 0] = (rgb - 0.5) / SH_C0
        rots = torch.zeros(n, 4, device=dev)
        rots[:, 0] = 1.0
        opac = torch.full((n,), math.log(0.1 / 0.9), device=dev)
        conf = torch.ones(n, device=dev)
        cat = (lambda old, new: torch.cat([old.detach(), new])) if append else (lambda old, new: new)
        p = lambda t: torch.nn.Parameter(t.contiguous())
        self._xyz, self._features = p(cat(self._xyz, pts)), p(cat(self._features, feats))
        self._scaling, self._rotation = p(cat(self._scaling, scales)), p(cat(self._rotation, rots))
        self._opacity = p(cat(self._opacity, opac))
        self.confidence = cat(self.confidence, conf)
        self.filter_3D = None                 # another set of Gaussians (GSTrainer.ensure_filter_3D computes it again)

    def to(self, device):
        """diffusionGS.py:901-907 moves the Gaussians off and back on the GPU around svd_render; with 288 GB of HBM
        nothing has to move — kept as a no-op-compatible method."""
        dev = torch.device(device)
        for name in ("_xyz", "_scaling", "_rotation", "_opacity", "_features"):
            t = getattr(self, name)
            t.data = t.data.to(dev)
        self.confidence = self.confidence.to(dev)
        if self.filter_3D is not None:
            self.filter_3D = self.filter_3D.to(dev)
        return self
