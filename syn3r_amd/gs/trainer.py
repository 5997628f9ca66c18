"""HOT LOOP A host side: the trainer surface `DiffusionGS` consumes
(`model/diffusionGS.py:51,132-139,154,166,1612-1641,1685-1697`), implemented on the HIP rasteriser.

The reference delegates all of this to `FSGS.utils.trainer_v4.GSTrainer` (un-vendored submodule): only the
call surface is visible.  This module provides that surface with the published 3DGS training step
(render -> (1-lambda) L1 + lambda (1-SSIM) photometric loss weighted by the camera confidence -> backward ->
Adam; the loss and the Adam update are the fused HIP operators of `train_ops`), no densification
heuristics (out of scope).

`GSTrainer` holds construction, the optimiser and its learning rate, camera registration, checkpoints, the two step routes and
the loop.  What it is made of lives beside it and is re-exported here: the cameras and their registry (`camera.py`), the Gaussians
(`gaussian_model.py`), the options and `expon_lr` (`params.py`); and five objects it owns, each with the state of one concern:
adaptive density control (`density.DensityControl`) and what takes its seat with `opt.mcmc` (`mcmc.MCMCControl`), the
camera-gradient table of pose refinement (`pose.PoseTable`), the 3D filter's camera table (`filter3d.Filter3DCache`) and the
per-camera exposure (`exposure.ExposureControl`).
"""
from __future__ import annotations

import math
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from .. import raster
from ..raster import GaussianRasterizationSettings, GaussianRasterizer
from .camera import Camera, _projection, _Scene, _world2view  # noqa: F401  (re-exported: callers import them from here)
from .density import DensityControl
from .exposure import CAMERA_KINDS as EXPOSURE_CAMERA_KINDS
from .exposure import ExposureControl
from .filter3d import Filter3DCache
from .gaussian_model import SH_C0, GaussianModel, build_rotation  # noqa: F401
from .mcmc import MCMCControl
from .params import OptimizationParams, expon_lr
from .pose import PoseTable
from .train_ops import FusedAdam, depth_correlation_loss, image_metrics, l1_loss, photometric_loss
from .train_ops import depth_correlation_local_loss, depth_correlation_local_loss_step
from .train_ops import depth_correlation_loss_step, exposure_apply, exposure_apply_step, l1_loss_step, photometric_loss_step
from .train_ops import depth_edge_weights as edge_weights_of_image
from .train_ops import depth_smoothness_loss, depth_smoothness_loss_step
from .train_ops import mcmc_noise, mcmc_reg_step
from .train_ops import photo_reprojection_loss, photo_reprojection_loss_step
from . import reproj as reproj_host


DEPTH_SMOOTH_CAMERA_KINDS = ("all", "train", "pseudo")


class GSTrainer:
    def __init__(self, gaussians: GaussianModel, train_cameras: Sequence[Camera], opt: Optional[OptimizationParams] = None,
                 background=(0.0, 0.0, 0.0), model_path: Optional[str] = None,
                 checkpoint_iterations: Optional[Sequence[int]] = None):
        self.gaussians, self.opt = gaussians, opt or OptimizationParams()
        self.scene = _Scene(train_cameras, model_path)
        self.dust3r = None                # injected: to(device) / [make_pairs] / run(frames, c2w_poses=, intrinsics=, preset_pairs=)
        self.flow_net = None              # injected: flow_net(image_a [3,H,W], image_b [3,H,W]) -> flow a->b [2,H,W] (GMFlow's role)
        self.lpips = None                 # injected: syn3r_amd.gs.lpips.LPIPS with loaded weights (the `lpips` package's role)
        self.depth_net = None             # injected: depth_net(image [3,H,W]) -> prior [H,W] (FSGS' monocular DPT / MiDaS role)
        self.checkpoint_iterations: List[int] = list(checkpoint_iterations or [])
        self.iteration = 0
        self.densify = False              # adaptive density control inside train_step (training / finetune set it)
        self.truncated_renders = 0        # renders whose (Gaussian, tile) pair list outgrew the async capacity (see _loop)
        self._ck_tag, self._ck_keys = None, []        # _capacity_keys
        if self.opt.pose_opt_cameras not in ("train", "pseudo", "all"):
            raise ValueError(f"OptimizationParams.pose_opt_cameras must be 'train', 'pseudo' or 'all', got {self.opt.pose_opt_cameras!r}")
        if self.opt.exposure_cameras not in EXPOSURE_CAMERA_KINDS:
            raise ValueError(f"OptimizationParams.exposure_cameras must be 'pseudo', 'train' or 'all', got {self.opt.exposure_cameras!r}")
        if self.opt.depth_smooth_cameras not in DEPTH_SMOOTH_CAMERA_KINDS:
            raise ValueError("OptimizationParams.depth_smooth_cameras must be 'all', 'train' or 'pseudo', got "
                             f"{self.opt.depth_smooth_cameras!r}")
        reproj_host.check_options(self.opt)
        if self.opt.mcmc:
            if self.opt.use_proximity_densify or self.opt.densify_abs_grad:
                raise ValueError("OptimizationParams.mcmc replaces the clone / split / prune control: use_proximity_densify and "
                                 "densify_abs_grad are rules of that control and cannot be combined with it")
            if int(self.opt.mcmc_cap_max) < int(gaussians._xyz.shape[0]):
                raise ValueError(f"OptimizationParams.mcmc_cap_max = {self.opt.mcmc_cap_max} is below the initial number of Gaussians, "
                                 f"{int(gaussians._xyz.shape[0])}")
        self.density = DensityControl(self)           # adaptive density control: every change of the set of Gaussians
        self.mcmc = MCMCControl(self)                 # `opt.mcmc`: relocation and growth to a cap in the density control's seat
        self.filter3d = Filter3DCache()               # `opt.filter_3d`: the camera table and the age of `gaussians.filter_3D`
        self.pose = PoseTable(self)                   # `opt.pose_opt`: the camera-gradient table and its counts
        self.exposure = ExposureControl(self)         # `opt.exposure_opt`: which cameras have an exposure, its gradient and its Adam step
        self.reproj = reproj_host.ReprojCache()       # `opt.reproj_weight`: per target its source views and their tables (not in checkpoints)
        self.background = torch.tensor(background, dtype=torch.float32, device=gaussians._xyz.device)
        self._rng = np.random.default_rng(self.opt.seed)
        self.reset_optimizers()

    # ------------------------------------------------------------------ public names of what the four owned objects keep and do
    # (the docstrings are at the implementations)
    last_unpooled = property(lambda self: self.density.last_unpooled, doc="Gaussians the proximity unpooling added in the last "
                             "densify_and_prune call")
    filter_3d_computes = property(lambda self: self.filter3d.computes, doc="how often ensure_filter_3D has computed the filter")
    pose_updates = property(lambda self: self.pose.updates, doc="camera moves applied so far (apply_pose_updates)")
    exposure_updates = property(lambda self: self.exposure.updates, doc="exposure (Adam) steps taken so far")

    def densify_and_prune(self, max_grad: float, min_opacity: float, extent: float, max_screen_size: Optional[float]):
        return self.density.densify_and_prune(max_grad, min_opacity, extent, max_screen_size)

    def reset_opacity(self):
        return self.density.reset_opacity()

    def proximity_unpool(self, extent: float) -> int:
        return self.density.proximity_unpool(extent)

    def ensure_filter_3D(self) -> Optional[torch.Tensor]:
        return self.filter3d.ensure(self.gaussians, self.opt, self.scene.train_cameras[1.0])

    def apply_pose_updates(self) -> int:
        return self.pose.apply()

    def flush_pose_updates(self) -> int:
        return self.pose.flush()

    def exposed(self, image: torch.Tensor, cam: Camera) -> torch.Tensor:
        """What the loss of a step on `cam` compares with the camera's target: E(image) for a camera that has an exposure
        (`opt.exposure_opt`, `gs/exposure.py`), else `image` itself.  Every render the trainer RETURNS is the scene colour."""
        return self.exposure.exposed(image, cam)

    # ------------------------------------------------------------------ surface used by DiffusionGS
    def reset_optimizers(self):
        """A fresh optimiser over the five parameter tensors (the published `training_setup`).  With `opt.feature_rest_lr_div`
        != 1 the features group carries the row split of `FusedAdam` (`lr_tail = feature_lr / div`, `row_len = 3 M`, `head_len
        = 3`): the published f_dc / f_rest groups on ONE tensor.  `opt.spatial_lr_scale` None is resolved here, to
        `cameras_extent()` of the cameras registered now."""
        g, o = self.gaussians, self.opt
        features = {"params": [g._features], "lr": o.feature_lr}
        if o.feature_rest_lr_div != 1.0:
            features.update(lr_tail=o.feature_lr / o.feature_rest_lr_div, row_len=3 * int(g._features.shape[1]), head_len=3)
        self.spatial_lr_scale = self.cameras_extent() if o.spatial_lr_scale is None else float(o.spatial_lr_scale)
        self.optimizer = FusedAdam([
            {"params": [g._xyz], "lr": o.position_lr}, features,
            {"params": [g._opacity], "lr": o.opacity_lr}, {"params": [g._scaling], "lr": o.scaling_lr},
            {"params": [g._rotation], "lr": o.rotation_lr}], eps=1e-15)

    def update_learning_rate(self, iteration: int) -> float:
        """Published `GaussianModel.update_learning_rate`: with `opt.position_lr_final` set, the xyz group's rate becomes
        spatial_lr_scale x expon_lr(iteration, position_lr, position_lr_final, ...) (host arithmetic into the `lr` the next launch
        carries; no launch, no synchronisation).  `iteration` is the loop's own 1-based counter (`train_step` passes
        `self.iteration + 1`), so the schedule restarts with every `training(0, ...)` / `finetune(0, ...)` - refine_GS resets the
        optimisers before each finetune anyway (diffusionGS.py:1634).  Whether FSGS' fork keeps one global step across refines is
        not visible: UNPINNED.  Returns the xyz group's rate."""
        o, grp = self.opt, self.optimizer.param_groups[0]
        if o.position_lr_final is not None:
            grp["lr"] = self.spatial_lr_scale * expon_lr(iteration, o.position_lr, o.position_lr_final, o.position_lr_delay_steps,
                                                         o.position_lr_delay_mult, o.position_lr_max_steps)
        return grp["lr"]

    def reset_gs(self):
        self.flush_pose_updates()
        return None

    @property
    def pseudo_cameras(self) -> List[Camera]:
        return self.scene.getPseudoCameras()

    def update_cameras(self, views, poses, K, cam_confidences, append: bool = True, load_iteration=None, confidence_maps=None):
        """diffusionGS.py:1631 — register SVD pseudo-views ([3,H,W] tensors + w2c poses) with their confidence in
        `scene.train_cameras` (appended, as the reference; the orchestrator restores the list after the finetune).
        `confidence_maps` (EXTENSION; default None): one per-pixel map ([H,W], see `Camera.confidence_map`) or None per view, a
        list of the length of `views`."""
        self.flush_pose_updates()                      # (pose refinement: what is pending belongs to the cameras registered so far)
        if np.isscalar(cam_confidences):
            cam_confidences = [float(cam_confidences)] * len(views)
        if confidence_maps is None:
            confidence_maps = [None] * len(views)
        elif len(confidence_maps) != len(views):
            raise ValueError(f"update_cameras: {len(confidence_maps)} confidence_maps for {len(views)} views")
        cams = [Camera.from_w2c(np.asarray(p), np.asarray(K), v.shape[1], v.shape[2], image=v, cam_confidence=c, confidence_map=m,
                                data_device=self.gaussians._xyz.device)
                for v, p, c, m in zip(views, poses, cam_confidences, confidence_maps)]
        for c in cams:
            c.is_pseudo = True
        for scale, lst in self.scene.train_cameras.items():
            keep = list(lst) if append else [c for c in lst if not getattr(c, "is_pseudo", False)]
            self.scene.train_cameras[scale] = keep + cams
        self.reproj.retain(self.scene.train_cameras[1.0])       # (a retired pseudo-view and its image must not live on in the source cache)

    # ---- checkpoints with the reference's file names (diffusionGS.py:1611-1625)
    def _ckpt_dir(self) -> str:
        if not self.scene.model_path:
            raise RuntimeError("GSTrainer: scene.model_path is not set (checkpoints need a directory)")
        os.makedirs(self.scene.model_path, exist_ok=True)
        return self.scene.model_path

    def save_checkpoint(self, iteration: int, refine_epoch: Optional[int] = None, latest: bool = False) -> str:
        """`chkpnt{iteration}.pth` after the initial training, `refine_{epoch}_chkpnt{iteration}.pth` after a finetune,
        `chkpnt_latest.pth` as the fallback the reference looks for: a `(capture, iteration)` tuple as published 3DGS."""
        name = "chkpnt_latest.pth" if latest else (f"chkpnt{iteration}.pth" if refine_epoch is None
                                                   else f"refine_{refine_epoch}_chkpnt{iteration}.pth")
        path = os.path.join(self._ckpt_dir(), name)
        state = self.gaussians.capture()
        if self.opt.pose_opt:
            # refined poses and their Adam state, per registered camera (key absent with the option off: the file it always was).  What
            # is pending in the gradient table is NOT applied here: saving must not change the run
            state["camera_poses"] = self.pose.capture()
        if self.opt.exposure_opt:
            # the exposures and their Adam state, per registered camera that has any (key absent with the option off)
            state["camera_exposures"] = self.exposure.capture()
        torch.save((state, int(iteration)), path)
        return path

    def load_checkpoint(self, checkpoint: str):
        """diffusionGS.py:1618,1624 — restore the Gaussians from a checkpoint file; optimiser state starts afresh
        (the orchestrator calls reset_optimizers right after, :1634).  The file is THIS repository's format — a
        `(dict of tensors / ints, iteration)` pair written by `save_checkpoint` under the reference's file names — and
        is read with the tensors-only loader (`weights_only=True`: no pickled code is executed).  FSGS' own
        `chkpnt*.pth` (a tuple of optimiser and model objects) is a different format and is rejected by that loader."""
        state, it = torch.load(checkpoint, map_location=self.gaussians._xyz.device, weights_only=True)
        self.gaussians.restore(state)
        self.iteration = int(it)
        if "camera_poses" in state:                    # (written with `opt.pose_opt`; an older file has no such key and loads as before)
            self.pose.restore(state["camera_poses"])
        if "camera_exposures" in state and self.opt.exposure_opt:      # (a trainer with the option off leaves the key alone)
            self.exposure.restore(state["camera_exposures"])
        self.reset_optimizers()

    def reset_gaussians_from_pcd(self, pcd, append_to_old_gaussians: bool = False):
        """diffusionGS.py:1685-1687 — re-initialise (or extend) the Gaussians from a dense point cloud: an object with
        `.points` / `.colors` (open3d) or a (points [n,3], colours [n,3] in [0,1]) pair."""
        if hasattr(pcd, "points"):
            pts, col = pcd.points, pcd.colors            # open3d-like cloud or syn3r_amd.pcd.PointCloud (device tensors)
        else:
            pts, col = pcd
        self.gaussians.set_from_pcd(pts, col, append=append_to_old_gaussians)
        self.reset_optimizers()

    def generate_corresp_mask(self, gs_renderings, svd_outputs, dist_thresh: float = 3, desc_only: bool = False):
        """diffusionGS.py:377 — per (Gaussian render, diffused frame) pair the mask of pixels with a consistent dense
        correspondence, and the flows.  FSGS' wrapper and its GMFlow network are absent; here the flow network is the
        injected attribute `flow_net` (called once per direction) and the test is the forward / backward cycle error below
        `dist_thresh` pixels (`syn3r_flow_cycle_mask`, csrc/warp.hip).  Images go to `flow_net` exactly as the orchestrator
        passes them ([3,H,W] tensors; the reference hands over the render in [0,1] and the diffused frame in [0,255]).
        Returns (masks, flow_bwfw): masks[i] is [1,H,W] fp32 in {0,1} (the caller reads `masks[0][0]`), flow_bwfw[i] the
        (forward, backward) flow pair."""
        if desc_only:
            raise NotImplementedError("desc_only=True (descriptor matching) is internal to FSGS; the orchestrator passes False")
        if self.flow_net is None:
            raise RuntimeError("generate_corresp_mask needs GSTrainer.flow_net (the optical-flow network, GMFlow in the reference)")
        assert len(gs_renderings) == len(svd_outputs)
        from ..pcd import flow_cycle_mask
        dev = self.gaussians._xyz.device
        masks, flows = [], []
        for a, b in zip(gs_renderings, svd_outputs):
            a, b = a.to(dev, torch.float32), b.to(dev, torch.float32)
            fw = torch.as_tensor(self.flow_net(a, b), dtype=torch.float32).to(dev)
            bw = torch.as_tensor(self.flow_net(b, a), dtype=torch.float32).to(dev)
            masks.append(flow_cycle_mask(fw[None], bw[None], float(dist_thresh)))
            flows.append((fw, bw))
        return masks, flows

    def find_nearest_cam(self, cams: Sequence[Camera], candidates: Sequence[Camera], multi_view_max_angle: float = 30.0,
                         multi_view_min_dis: float = 0.01, multi_view_max_dis: float = 1.5, multi_view_num: int = 8):
        """diffusionGS.py:475-477 (only reached from the dead `_extrapolate_from_gs`; FSGS source absent, so this follows
        the public multi-view neighbour selection it is named after — UNPINNED): for every camera the candidates
        whose viewing direction is within `multi_view_max_angle` degrees and whose centre is within
        [min_dis, max_dis], nearest first; stored as `cam.nearest_id` and returned."""
        out = []
        c_pos = np.stack([c.camera_center.detach().cpu().numpy() for c in candidates]) if len(candidates) else np.zeros((0, 3))
        c_dir = np.stack([np.asarray(c.R)[:, 2] for c in candidates]) if len(candidates) else np.zeros((0, 3))
        for cam in cams:
            pos, d = cam.camera_center.detach().cpu().numpy(), np.asarray(cam.R)[:, 2]
            dis = np.linalg.norm(c_pos - pos[None], axis=1)
            cosang = np.clip(c_dir @ d / (np.linalg.norm(c_dir, axis=1) * np.linalg.norm(d) + 1e-12), -1, 1)
            ang = np.degrees(np.arccos(cosang))
            ok = (ang < multi_view_max_angle) & (dis > multi_view_min_dis) & (dis < multi_view_max_dis)
            order = [int(i) for i in np.argsort(dis) if ok[i]][:multi_view_num]
            cam.nearest_id = order
            out.append(order)
        return out

    def evaluate(self, cams: Optional[Sequence[Camera]] = None) -> dict:
        """PSNR / SSIM of the current Gaussians over held-out (or the training) cameras, computed on the device
        (`train_ops.image_metrics`): the psnr / ssim columns of the per-scene record (SURVEY.md §8e;
        scripts/summarize_dl3dv.py:11-80 tabulates them).  LPIPS is reported when the trainer holds an `lpips` model
        (weights supplied by the caller), NaN otherwise.
        The cameras are rendered at the poses THEY hold.  With `opt.pose_opt` the training cameras have moved and with them, slightly,
        the frame the Gaussians live in; held-out test poses are NOT aligned to that refined frame (test-time pose alignment, as
        pose-refining papers evaluate, is out of scope), so their metrics carry the residual misalignment."""
        cams = list(cams) if cams is not None else self.scene.getTrainCameras()
        ps, ss, ls = [], [], []
        with torch.no_grad():
            for cam in cams:
                img = self.render_view(cam)["render"].clamp(0, 1)
                m = image_metrics(img, cam.original_image)
                ps.append(m[0])
                ss.append(m[1])
                if self.lpips is not None:
                    ls.append(self.lpips(img, cam.original_image))
        p, s_ = torch.stack(ps).mean(), torch.stack(ss).mean()
        lp = float(torch.stack(ls).mean()) if ls else float("nan")
        return {"psnr": float(p), "ssim": float(s_), "lpips": lp, "n": len(cams)}

    def cameras_extent(self) -> float:
        """Radius of the training cameras around their centroid x 1.1 (published `getNerfppNorm`)."""
        cams = self.scene.getTrainCameras()
        if not cams:
            return 1.0
        c = torch.stack([cam.camera_center.detach().float().cpu() for cam in cams])
        return float((c - c.mean(0, keepdim=True)).norm(dim=1).max() * 1.1) or 1.0

    def _raster_settings(self, cam: Camera, scale_modifier: float) -> GaussianRasterizationSettings:
        return GaussianRasterizationSettings(
            image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
            tanfovy=math.tan(cam.FoVy * 0.5), bg=self.background, scale_modifier=scale_modifier,
            viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=self.gaussians.active_sh_degree,
            campos=cam.camera_center, prefiltered=False, debug=False, antialiasing=bool(self.opt.antialiasing))

    def render_view(self, cam: Camera, scaling_modifier: float = 1.0, _pose_row: Optional[int] = None):
        """-> {'render' [3,H,W], 'depth' [1,H,W], 'alpha' [1,H,W], ...} (diffusionGS.py:154-172).
        `_pose_row` (train_step alone, `opt.pose_opt`): the backward of this render ADDS its camera gradient to that row of the table."""
        g = self.gaussians
        f3 = self.ensure_filter_3D()
        means2D = torch.zeros_like(g.get_xyz, requires_grad=True)
        extra = {}
        if self.opt.densify_abs_grad:
            # AbsGS: the backward of this render fills the buffer (zeros until then, and for a render that is never differentiated)
            extra["viewspace_abs_grad"] = torch.zeros((g.get_xyz.shape[0], 2), dtype=torch.float32, device=g.get_xyz.device)
        color, radii, depth, alpha = GaussianRasterizer(self._raster_settings(cam, scaling_modifier))(
            g.get_xyz, means2D, g.get_opacity, shs=g.get_features, scales=g.get_scaling, rotations=g.get_rotation,
            confidence=g.confidence, filter_3D=f3, means2D_abs=extra.get("viewspace_abs_grad"),
            camera_grad=None if _pose_row is None else self.pose.table[_pose_row], camera_grad_accumulate=True)
        return {"render": color, "depth": depth, "alpha": alpha, "viewspace_points": means2D, "visibility_filter": radii > 0,
                "radii": radii, **extra}

    def _pick_camera(self) -> Camera:
        pseudo = self.scene.getPseudoCameras()
        if pseudo and self._rng.random() < self.opt.pseudo_cam_sampling_rate:
            return pseudo[int(self._rng.integers(len(pseudo)))]
        cams = self.scene.getTrainCameras()
        return cams[int(self._rng.integers(len(cams)))]

    def depth_prior(self, cam: Camera) -> Optional[torch.Tensor]:
        """The camera's monocular depth prior [H,W] fp32: `cam.depth_image`, else `depth_net(cam.original_image)` computed ONCE under
        no_grad and cached on the camera (pseudo-views registered by `update_cameras` included); None without either."""
        if getattr(cam, "depth_image", None) is None:
            if self.depth_net is None or cam.original_image is None:
                return None
            with torch.no_grad():
                d = torch.as_tensor(self.depth_net(cam.original_image), dtype=torch.float32).to(cam.original_image.device)
            cam.depth_image = (d[0] if d.dim() == 3 and d.shape[0] == 1 else d).detach().contiguous()
        return cam.depth_image

    # ------------------------------------------------------------------ the loss of one step, assembled once for the two routes
    def _depth_term_prior(self, cam: Camera) -> Optional[torch.Tensor]:
        """The prior of a step on `cam` when either depth-correlation term is on (None: neither, or a camera without a prior)"""
        return self.depth_prior(cam) if self.opt.depth_weight > 0.0 or self.opt.depth_local_weight > 0.0 else None

    def depth_patch_origin(self, cam: Camera, iteration: Optional[int] = None) -> Tuple[int, int]:
        """The origin (oy, ox) of the patch grid of `opt.depth_local_weight` for a step on `cam` at `iteration` (default: the
        current one).  With `opt.depth_patch_jitter` it is drawn uniformly from [0, min(P, H - P + 1)) x [0, min(P, W - P + 1)) -
        at least one full patch always fits - by a generator seeded with (`opt.seed`, iteration) ALONE: not `self._rng`, so the
        camera-pick sequence is the one of a run without the term, a resumed run continues the sequence, and a checkpoint holds
        nothing new.  Without jitter (0, 0).  The rule is chosen, not taken from a source: UNPINNED."""
        P, H, W = int(self.opt.depth_patch_size), int(cam.image_height), int(cam.image_width)
        if H < P or W < P:
            raise ValueError(f"OptimizationParams.depth_patch_size = {P} does not fit a {H} x {W} camera: the patch-wise depth term "
                             "needs at least one full patch")
        if not self.opt.depth_patch_jitter:
            return 0, 0
        it = self.iteration if iteration is None else int(iteration)
        rng = np.random.default_rng([int(self.opt.seed) & (2 ** 64 - 1), it])
        return int(rng.integers(min(P, H - P + 1))), int(rng.integers(min(P, W - P + 1)))

    def depth_edge_weights(self, cam: Camera) -> torch.Tensor:
        """The edge weights [2,H,W] of the depth-smoothness term for `cam`: the caller's own (`cam.depth_edge_weights`, never
        recomputed), else `train_ops.depth_edge_weights(cam.original_image, opt.depth_smooth_gamma)` computed ONCE under no_grad and
        cached on the camera with the gamma and the image (its identity and version) they were made from; recomputed when either
        changes.  8 bytes per pixel per camera."""
        own = getattr(cam, "depth_edge_weights", None)
        if own is not None:
            return own
        image, gamma = cam.original_image, float(self.opt.depth_smooth_gamma)
        if image is None:
            raise ValueError("depth_edge_weights: the camera has no original_image")
        c = getattr(cam, "_depth_edge_cache", None)
        if c is None or c[0] != gamma or c[1] is not image or c[2] != image._version:
            with torch.no_grad():
                c = (gamma, image, image._version, edge_weights_of_image(image, gamma))
            cam._depth_edge_cache = c
        return c[3]

    def _depth_smooth_weights(self, cam: Camera) -> Optional[torch.Tensor]:
        """The edge weights of a step on `cam` when the depth-smoothness term acts on it (None: the term is off, the camera is not of
        `opt.depth_smooth_cameras`, or it has no target image).  Touches neither `depth_prior` nor `depth_net`."""
        if not self.opt.depth_smooth_weight > 0.0:
            return None
        kind = self.opt.depth_smooth_cameras
        if kind not in DEPTH_SMOOTH_CAMERA_KINDS:
            raise ValueError(f"OptimizationParams.depth_smooth_cameras must be 'all', 'train' or 'pseudo', got {kind!r}")
        pseudo = bool(getattr(cam, "is_pseudo", False))
        if (kind == "train" and pseudo) or (kind == "pseudo" and not pseudo) or cam.original_image is None:
            return None
        return self.depth_edge_weights(cam)

    def _reproj_sources(self, cam: Camera):
        """The sources of a step on `cam` when the reprojection term acts on it at this iteration: (source images, `ReprojViews`,
        source cameras) from the per-target cache (`gs/reproj.py`), else None - the term is off, the iteration is before
        `opt.reproj_from_iter`, the camera is not of `opt.reproj_cameras`, has no target image, or no input view passes the source rule."""
        return reproj_host.sources_for(self.reproj, self.opt, cam, self.scene.getTrainCameras(), self.iteration)

    def _photo_loss(self, image: torch.Tensor, cam: Camera, with_grad: bool):
        """The photometric term of a step on `cam`: the scalar weight is `cam.cam_confidence`, the per-pixel one `cam.confidence_map`
        (None: none), `opt.lambda_dssim` > 0 takes the D-SSIM loss and 0 plain L1.  `with_grad` (the explicit route): the operators
        without autograd, -> (loss, d loss / d image); else (the autograd route) the autograd ones, -> (loss, None)."""
        w, wmap, lam = float(cam.cam_confidence), getattr(cam, "confidence_map", None), self.opt.lambda_dssim
        if with_grad:
            if lam > 0.0:
                loss, _, d_image = photometric_loss_step(image, cam.original_image, lam, w, weight_map=wmap)
                return loss, d_image
            return l1_loss_step(image, cam.original_image, w, weight_map=wmap)
        if lam > 0.0:
            return photometric_loss(image, cam.original_image, lam, w, weight_map=wmap), None
        return l1_loss(image, cam.original_image, weight=w, weight_map=wmap), None

    def _explicit_step(self, cam: Camera) -> Tuple[torch.Tensor, dict]:
        """One optimisation step WITHOUT autograd: raw parameters in, raw-parameter gradients out.  The activations and
        their chain rule run INSIDE the rasteriser's projection kernels (`syn3r_raster_preprocess_raw` / `_backward_raw`, round 6:
        `syn3r_gaussian_activate[_backward]`'s arithmetic, two launches and six intermediate tensors less per iteration; the
        autograd path keeps torch's three operators), the loss' value and gradient are `syn3r_photo_loss_step`'s two launches,
        and no screen-space `means2D` tensor is allocated per render.  Same arithmetic as the autograd path
        (`tests/test_trainer_gpu.py` holds one step of each against the oracle and against each other)."""
        g = self.gaussians
        # this step discards the rasteriser's confidence gradient: the per-Gaussian confidence is data here, as in the call sites
        # (model/diffusionGS.py:139,1640); a trainable one has to take the autograd path
        conf = g.confidence
        if conf is not None and getattr(conf, "requires_grad", False):
            raise ValueError("_explicit_step: a confidence tensor that requires grad needs train_step(explicit=False)")
        prior = self._depth_term_prior(cam)
        edge = self._depth_smooth_weights(cam)
        rsrc = self._reproj_sources(cam)
        f3 = self.ensure_filter_3D()
        with torch.no_grad():
            # log-scales / raw quaternions / logits in, THEIR gradients out (syn3r_raster_*_raw)
            color, radii, depth, alpha, rstate = raster.rasterize_forward(g._xyz, g._features, g._opacity, g._scaling, g._rotation,
                                                                          g.confidence, self._raster_settings(cam, 1.0), raw_params=True,
                                                                          filter_3D=f3)
            A = self.exposure.state(cam)              # None: a camera without an exposure runs the plain step, launch for launch
            loss, d_color = self._photo_loss(color if A is None else exposure_apply_step(color, A), cam, True)
            if A is not None:                         # d loss / d E(color) -> d loss / d color; d loss / d A into the control's buffer,
                d_color = self.exposure.backward(color, cam, d_color)       # then ITS Adam step (no host read)
                self.exposure.step(cam)
            d_depth = None
            if prior is not None and self.opt.depth_weight > 0.0:
                d_loss, d_depth = depth_correlation_loss_step(depth, prior, self.opt.depth_weight, self.opt.depth_offset)
                loss = loss + d_loss
            if prior is not None and self.opt.depth_local_weight > 0.0:        # ADDED into the global term's buffer when both are on
                d_loss, d_depth = depth_correlation_local_loss_step(depth, prior, self.opt.depth_local_weight, self.opt.depth_patch_size,
                                                                    self.depth_patch_origin(cam), self.opt.depth_offset, grad_out=d_depth)
                loss = loss + d_loss
            if edge is not None:                      # prior-free smoothness: ADDED into the buffer of the terms above when one is on
                d_loss, d_depth = depth_smoothness_loss_step(depth, edge, self.opt.depth_smooth_weight, grad_out=d_depth)
                loss = loss + d_loss
            d_alpha = None
            if rsrc is not None:                      # reprojection: depth gradient ADDED into the buffer above, the alpha gradient is new
                d_loss, d_depth, d_alpha = photo_reprojection_loss_step(depth, alpha, cam.original_image, rsrc[0], rsrc[1],
                                                                        self.opt.reproj_weight, self.opt.reproj_alpha_min,
                                                                        grad_out=d_depth)
                loss = loss + d_loss
            extra = {}
            if self.opt.densify_abs_grad:             # (uninitialised: the backward writes every row)
                extra["viewspace_abs_grad"] = torch.empty((g._xyz.shape[0], 2), dtype=torch.float32, device=g._xyz.device)
            pose_row = self.pose.row(cam)             # the camera gradient of this step is ADDED to the camera's row: no host read here
            d_m3, d_m2, d_sh, d_lg, d_ls, d_rr, _ = raster.rasterize_backward(
                rstate, d_color, d_depth, d_alpha, abs_grad_out=extra.get("viewspace_abs_grad"),
                camera_grad_out=None if pose_row is None else self.pose.table[pose_row], camera_grad_accumulate=True)
            self.pose.count(pose_row)
            g._xyz.grad, g._features.grad, g._opacity.grad, g._scaling.grad, g._rotation.grad = d_m3, d_sh, d_lg.reshape(g._opacity.shape), d_ls, d_rr
            if self.opt.mcmc:                         # the two L1 regularisers: values to the loss, gradients ADDED to the raw ones
                reg = mcmc_reg_step(g._opacity.detach(), g._scaling.detach(), self.opt.mcmc_opacity_reg, self.opt.mcmc_scale_reg,
                                    g._opacity.grad, g._scaling.grad)
                loss = loss + (reg[0] + reg[1])
        out = {"render": color, "depth": depth, "alpha": alpha, "viewspace_grad": d_m2, "visibility_filter": None,      # visible = radii > 0: add_densification_stats takes it from `radii` on the device
               "radii": radii, **extra}
        return loss, out

    def _autograd_step(self, cam: Camera, lpips_on: bool = False) -> Tuple[torch.Tensor, dict]:
        """One optimisation step THROUGH autograd (`render_view`, the autograd operators of `train_ops`, `loss.backward()`): the
        route of the LPIPS term (`lpips_on`) and of a trainable confidence.  `out` is `render_view`'s dictionary: its boolean
        `visibility_filter` and the gradient on `viewspace_points` are what the density control reads on this route."""
        pose_row = self.pose.row(cam)
        out = self.render_view(cam, _pose_row=pose_row)
        A = self.exposure.state(cam)                  # None: a camera without an exposure
        if A is not None:
            A = A.detach().requires_grad_(True)       # (a leaf over `cam.exposure`'s memory; its gradient goes to `exposure.step` below)
        image = out["render"] if A is None else exposure_apply(out["render"], A)       # the photometric and LPIPS terms see E(render)
        loss, _ = self._photo_loss(image, cam, False)
        if lpips_on:
            # the perceptual term of the refine stage (diffusionGS.py:1690,1697; `--lpips_weight`): published LPIPS-VGG on the
            # whole render, weighted like the photometric term by the camera confidence.  How FSGS applies it is not visible
            # (un-vendored): UNPINNED.
            loss = loss + (self.opt.lpips_weight * float(cam.cam_confidence)) * self.lpips(image.clamp(0, 1), cam.original_image)
        prior = self._depth_term_prior(cam)
        if prior is not None and self.opt.depth_weight > 0.0:
            loss = loss + depth_correlation_loss(out["depth"], prior, self.opt.depth_weight, self.opt.depth_offset)
        if prior is not None and self.opt.depth_local_weight > 0.0:
            loss = loss + depth_correlation_local_loss(out["depth"], prior, self.opt.depth_local_weight, self.opt.depth_patch_size,
                                                       self.depth_patch_origin(cam), self.opt.depth_offset)
        edge = self._depth_smooth_weights(cam)
        if edge is not None:
            loss = loss + depth_smoothness_loss(out["depth"], edge, self.opt.depth_smooth_weight)
        rsrc = self._reproj_sources(cam)
        if rsrc is not None:
            loss = loss + photo_reprojection_loss(out["depth"], out["alpha"], cam.original_image, rsrc[0], rsrc[1],
                                                  self.opt.reproj_weight, self.opt.reproj_alpha_min)
        if self.opt.mcmc:                             # the two L1 regularisers on the plain opacity and scales (not the filter_3d ones)
            g = self.gaussians
            loss = loss + (self.opt.mcmc_opacity_reg * g.get_opacity.mean() + self.opt.mcmc_scale_reg * g.get_scaling.mean())
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.pose.count(pose_row)
        if A is not None:
            self.exposure.step(cam, A.grad)
        return loss, out

    def train_step(self, cam: Optional[Camera] = None, explicit: Optional[bool] = None) -> torch.Tensor:
        """One optimisation step; returns the loss as a DEVICE scalar (no host synchronisation: the loop queues
        iterations back to back, `float(loss)` is the caller's choice).  `opt.use_lpips_loss` (set by the orchestrator
        around refine_GS, diffusionGS.py:1690,1697) adds `opt.lpips_weight` x LPIPS-VGG (`syn3r_amd.gs.lpips`, HIP) when the
        trainer has been given an `lpips` model with weights (the pretrained ones are not reachable offline: the caller
        loads them, as for CLIP / VAE / UNet); without one the switch is inert.
        `opt.depth_weight` > 0 adds FSGS' depth-correlation term `depth_weight * (1 - Pearson(rendered depth, prior))` (the better of
        its two prior transforms, `train_ops.depth_correlation_loss`) for a camera with a prior (`depth_prior`: `cam.depth_image` or
        the injected `depth_net`); a camera without one skips it.  As FSGS' `loss += depth_weight * depth_loss` the term is weighted
        by `depth_weight` alone, not by the camera confidence - UNPINNED for SYN3R's FSGS fork (not vendored).
        `opt.depth_local_weight` > 0 (EXTENSION, default off: every launch is what it was) adds the same term PATCH-WISE next to it,
        `depth_local_weight` x the mean over `opt.depth_patch_size` pixel patches of (1 - Pearson) per patch
        (`train_ops.depth_correlation_local_loss`: two more launches), on both routes and for the same cameras, weighted by
        `depth_local_weight` alone; the patch grid's origin is `depth_patch_origin`'s.  A camera smaller than the patch on a side is a
        ValueError.  On the explicit route its gradient is added into the global term's buffer when both are on.
        `opt.depth_smooth_weight` > 0 (EXTENSION, default off: every launch is what it was) adds the prior-free edge-aware smoothness
        term `depth_smooth_weight` x (S_x + S_y) / mean depth after the two Pearson terms (`train_ops.depth_smoothness_loss`: two more
        launches; S the mean of exp(-`depth_smooth_gamma` |target image difference|) |rendered depth difference| over a direction's
        pixel pairs), on both routes, for the cameras of `opt.depth_smooth_cameras` ("all", "train", "pseudo") that have an
        `original_image`.  It needs no prior: `depth_prior` / `depth_net` are not touched by it, so pseudo-views are regularised as
        well.  The edge weights come from `depth_edge_weights(cam)` (once per camera, cached on it).  Weighted by
        `depth_smooth_weight` alone, not by the camera confidence or its map.  On the explicit route its gradient is added into the
        Pearson terms' buffer when one of them made one.  gamma = 1 and the division by the mean are recalled from Monodepth2: UNPINNED.
        `opt.reproj_weight` > 0 (EXTENSION, default off: every launch is what it was) adds the multi-view photometric reprojection
        term after the smoothness term (`train_ops.photo_reprojection_loss`: two more launches), on both routes: the rendered depth
        along the ray, depth / alpha, carries each pixel of the target into up to `opt.reproj_sources` other input views, and
        `reproj_weight` x the mean over the live pixels of the smallest L1 difference between the colour found there and the
        target's own is the loss (Monodepth2's minimum reprojection error, no SSIM, no auto-mask: UNPINNED).  It acts on the cameras
        of `opt.reproj_cameras` from iteration `opt.reproj_from_iter` on; sources are input views chosen by `gs/reproj.py`'s rule
        (same size, viewing direction within `opt.reproj_max_angle` degrees, nearest first) and cached per target until a pose or the
        camera list changes; a target without a source skips the term.  Weighted by `reproj_weight` alone, not by the camera
        confidence or its map, and it compares the RAW images: the exposure transform does not touch it.  It has gradients for
        depth AND alpha: on the explicit route the depth gradient is added into the buffer of the terms before it when one of them
        made one, the alpha gradient is a new buffer, and `rasterize_backward` is handed a `g_alpha` only on a step on which the
        term ran.  Out of scope: a gradient through the relative views (with `opt.pose_opt` the term sees the moved poses, and its
        depth and alpha gradients reach the target's pose through the render as any depth gradient does, but how q depends on the poses
        is not differentiated), exposure compensation between input views, an occlusion test against a second render.
        `cam.confidence_map` (EXTENSION, default None: the scalar-only, reference-shaped loss): a per-pixel weight on the photometric
        term (L1 and D-SSIM, `train_ops.photometric_loss(weight_map=)`) on top of the scalar `cam.cam_confidence`, on both the
        explicit and the autograd path.  The depth-correlation and LPIPS terms are NOT touched by the map.
        `opt.exposure_opt` (EXTENSION, default off: every launch is what it was): a camera of `opt.exposure_cameras` holds an affine
        colour transform `cam.exposure` (`gs/exposure.py`); the photometric and LPIPS terms compare E(render) with its target and the
        transform takes one Adam step per step on its camera, on both routes (four more launches: apply, the backward's two, Adam).
        The depth-correlation term and every render the trainer returns keep the scene colour; `exposed` shows what the loss saw.
        `opt.mcmc` (EXTENSION, default off: every launch is what it was): 3DGS-MCMC (`gs/mcmc.py`, csrc/mcmc.hip).  The loss gains
        `mcmc_opacity_reg` x mean opacity + `mcmc_scale_reg` x mean scale (`syn3r_mcmc_reg_step` after the rasteriser backward on the
        explicit route, torch operators on the autograd one), `mcmc.MCMCControl` takes the density control's seat (a step on which it
        ran skips the optimiser step), and after the optimiser step EVERY step adds the position noise `syn3r_mcmc_noise` with scale
        `mcmc_noise_lr` x the position group's current rate (0: no launch).  All read the plain scales and opacity.
        `explicit` (default: whenever the LPIPS term is off): the step without autograd (`_explicit_step`).
        The published schedule, when switched on (`OptimizationParams`): `update_learning_rate(iteration + 1)` before the optimiser
        step, `oneupSHdegree()` after every `sh_degree_interval`-th step (the published loop raises it at the top of the next
        iteration); the step both count is the loop's own counter `self.iteration` - UNPINNED, see `update_learning_rate`."""
        cam = cam or self._pick_camera()
        lpips_on = self.opt.use_lpips_loss and self.opt.lpips_weight > 0.0 and self.lpips is not None
        if explicit is None:
            explicit = not lpips_on
        if explicit:
            if lpips_on:
                raise ValueError("train_step(explicit=True) has no LPIPS term: the perceptual loss runs through autograd")
            loss, out = self._explicit_step(cam)
        else:
            loss, out = self._autograd_step(cam, lpips_on)
        changed = False
        if self.densify and self.opt.mcmc:
            changed = self.mcmc.control(out)  # (True when it ran: a relocation in place changes the set as an append does)
        elif self.densify:
            n0 = self.gaussians._xyz.shape[0]
            self.density.control(out)
            changed = self.gaussians._xyz.shape[0] != n0
        lr_xyz = self.update_learning_rate(self.iteration + 1)
        if not changed:                       # (the gradients of this step belong to the old set of Gaussians)
            self.optimizer.step()
        if self.opt.mcmc and self.opt.mcmc_noise_lr != 0.0:
            g = self.gaussians                # SGLD exploration: every step, after the optimiser's, on the plain scales and opacity
            with torch.no_grad():
                mcmc_noise(g._xyz.detach(), g._scaling.detach(), g._rotation.detach(), g._opacity.detach(),
                           float(self.opt.mcmc_noise_lr) * float(lr_xyz), int(self.opt.seed), self.iteration + 1)
        self.iteration += 1
        self.filter3d.tick()                  # (ensure_filter_3D: steps since the filter was computed)
        o = self.opt
        if o.pose_opt and self.iteration >= int(o.pose_opt_from_iter) and self.iteration % max(int(o.pose_opt_interval), 1) == 0:
            self.apply_pose_updates()         # (whether or not the density control changed the set: the gradient belongs to the camera)
        if self.opt.sh_degree_interval > 0 and self.iteration % self.opt.sh_degree_interval == 0:
            self.gaussians.oneupSHdegree()
        return loss.detach()

    def _capacity_keys(self):
        """The (device, N, H, W) keys of the binning capacities the training cameras use; the camera list is walked once per
        list object and Gaussian count, not per iteration."""
        g = self.gaussians
        dev, n = g._xyz.device, g._xyz.shape[0]
        cams = self.scene.train_cameras[1.0]
        tag = (id(cams), len(cams), n)
        if self._ck_tag != tag:
            shapes = sorted({(int(c.image_height), int(c.image_width)) for c in cams})
            self._ck_tag, self._ck_keys = tag, [raster.capacity_key(dev, n, h, w) for h, w in shapes]
        return self._ck_keys

    def _loop(self, first_iter: int, n: int) -> float:
        prev = raster.get_pair_count_mode()
        # async mode sizes the binning buffer from earlier renders of the same (N, H, W): one exact (sync) render per
        # camera first, so the capacity covers the view with the most (Gaussian, tile) pairs with 2x headroom
        raster.set_pair_count_mode("sync")
        if n > first_iter:
            with torch.no_grad():
                for cam in self.scene.train_cameras[1.0]:
                    self.render_view(cam)
        raster.set_pair_count_mode("async")          # no host round trip per render inside the loop
        self.iteration = first_iter                  # the density-control schedule counts from the start of this loop
        last = None

        def late_overflow(e):                        # an EARLIER render outgrew its pair capacity (reported late, see raster)
            if "async pair-count" not in str(e):
                raise e
            self.truncated_renders += int(getattr(e, "truncated", 1))

        try:
            for _ in range(first_iter, n):
                keys0 = self._capacity_keys() if self.densify else None
                cam = self._pick_camera()            # drawn ONCE per iteration: a retry renders the same view
                for attempt in range(4):
                    try:
                        last = self.train_step(cam)
                        break
                    except L.Syn3rError as e:        # raised by the render at the TOP of this step, about an earlier render
                        late_overflow(e)             # (whose step was applied): counted, reported in the scene record
                        if attempt == 3:             # (`truncated_renders`), the capacity raised - this iteration runs now;
                            raise                    # a retry may find ANOTHER pending truncated render: bounded
                if keys0 is not None:
                    keys1 = self._capacity_keys()
                    if keys1 != keys0:               # densification changed N: every (N, H, W) key is new.  Check what
                        try:                         # the old shapes still owe, then seed the new capacity from the old
                            raster.flush_pair_checks()           # one scaled by N_new / N_old (max over cameras is kept)
                        except L.Syn3rError as e:
                            late_overflow(e)
                        for k0, k1 in zip(keys0, keys1):
                            raster.carry_capacity(k0, k1, k1[1] / max(k0[1], 1))
            try:
                raster.flush_pair_checks()           # every remaining render's pair list was complete
            except L.Syn3rError as e:
                late_overflow(e)
        finally:
            raster.set_pair_count_mode(prev)
        return float(last) if last is not None else 0.0     # ONE synchronisation, at the end of the loop

    def _run(self, first_iter: int, iterations: Optional[int], disable_densification: bool) -> Tuple[int, float]:
        """The common head of `training` and `finetune`: -> (the iteration the loop ran to, its last loss)"""
        n = iterations if iterations is not None else self.opt.iterations
        self.densify = not disable_densification
        return n, self._loop(first_iter, n)

    def training(self, first_iter: int = 0, epoch_indicator: int = 0, iterations: Optional[int] = None,
                 disable_densification: bool = False):
        """HOT LOOP A (diffusionGS.py:139): `opt.iterations` optimisation steps with the published adaptive density
        control (clone / split / prune every `densification_interval` iterations from `densify_from_iter` on, opacity
        reset every `opacity_reset_interval`), then the checkpoints the orchestrator's refine_GS looks for
        (`chkpnt{N}.pth` for the configured checkpoint iterations, else `chkpnt_latest.pth`, diffusionGS.py:1620-1624)
        when `scene.model_path` is set."""
        n, last = self._run(first_iter, iterations, disable_densification)
        if self.scene.model_path:
            if n in self.checkpoint_iterations:
                self.save_checkpoint(n)
            self.save_checkpoint(n, latest=True)
        return last

    def finetune(self, first_iter: int = 0, refine_epoch: int = 0, disable_densification: bool = False,
                 pseudo_cam_sampling_rate: Optional[float] = None, iterations: Optional[int] = None):
        """diffusionGS.py:1640 — same loop (density control unless `disable_densification`, the flag refine_GS forwards,
        :1610), now also sampling the confidence-weighted pseudo-views; writes
        `refine_{epoch}_chkpnt{N}.pth` (the file the next cycle's refine_GS reloads, :1611-1618)."""
        if pseudo_cam_sampling_rate is not None:
            self.opt.pseudo_cam_sampling_rate = pseudo_cam_sampling_rate
        n, last = self._run(first_iter, iterations, disable_densification)
        if self.scene.model_path:
            self.save_checkpoint(n, refine_epoch=refine_epoch)
        return last
