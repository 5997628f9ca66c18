"""The options of the trainer (`gs/trainer.py`) and the published learning-rate schedule."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional


@dataclass
class OptimizationParams:
    iterations: int = 10_000
    position_lr: float = 1.6e-4
    feature_lr: float = 2.5e-3
    opacity_lr: float = 5e-2
    scaling_lr: float = 5e-3
    rotation_lr: float = 1e-3
    lambda_dssim: float = 0.2          # published 3DGS: L = (1 - lambda) L1 + lambda (1 - SSIM)
    pseudo_cam_sampling_rate: float = 0.02
    seed: int = 0
    use_lpips_loss: bool = False       # toggled by DiffusionGS.run (diffusionGS.py:1690,1697); see GSTrainer.train_step
    lpips_weight: float = 0.0
    # FSGS' depth-correlation term (GSTrainer.train_step): weight 0 = off; `depth_offset` is the c of its 1 / (prior + c) branch
    depth_weight: float = 0.0
    depth_offset: float = 200.0
    # The same term PATCH-WISE (EXTENSION after SparseGS' patch-based Pearson / DNGaussian's local depth normalisation; a monocular
    # prior is consistent only locally): `depth_local_weight` x the mean over the `depth_patch_size`-pixel square patches of a grid
    # of (1 - Pearson) per patch (`train_ops.depth_correlation_local_loss`), next to the global term; weight 0 = off.  The patch
    # size and the jitter rule are CHOSEN here, not taken from a source: UNPINNED, and resolution dependent (32 px suits the
    # 72 x 128 .. 1080p views this trainer sees; scale it with the image).  `depth_patch_jitter`: the grid's origin is drawn per
    # step from (seed, iteration) alone, so patch borders do not stay on the same pixels; False keeps the origin at (0, 0).
    depth_local_weight: float = 0.0
    depth_patch_size: int = 32
    depth_patch_jitter: bool = True
    # Prior-free edge-aware depth smoothness (EXTENSION: the reference has none; Monodepth2's form, which DNGaussian-, SparseGS- and
    # RegNeRF-style sparse-view pipelines use as well): `depth_smooth_weight` x (S_x + S_y) / mean depth, S the mean over a direction's
    # pixel pairs of exp(-gamma |target image difference|) x |rendered depth difference| (`train_ops.depth_smoothness_loss`,
    # csrc/depth_smooth.hip).  It needs the camera's own target image alone - no `depth_image`, no `depth_net` - so it acts on
    # pseudo-views as well.  `depth_smooth_cameras`: "all", "train" (the input views) or "pseudo" (the views `update_cameras`
    # registered).  The edge weights are computed once per camera and cached on it (8 bytes per pixel).  Weighted by
    # `depth_smooth_weight` alone, not by the camera confidence or its map, as the other depth terms.  gamma = 1 and the division by
    # the mean are RECALLED from Monodepth2, which is not available to check against: UNPINNED.  Weight 0 = off: every launch,
    # gradient, checkpoint and decision is what it was.  Nothing of it goes into checkpoints.
    depth_smooth_weight: float = 0.0
    depth_smooth_gamma: float = 1.0             # recalled, UNPINNED
    depth_smooth_cameras: str = "all"
    # Multi-view photometric reprojection (EXTENSION: the reference has none; Monodepth2's per-pixel minimum reprojection error, which
    # unsupervised-MVS and MVS-guided sparse-view 3DGS pipelines use as well): the depth rendered for a target view, taken along the
    # ray as z = depth / alpha, carries each pixel into up to `reproj_sources` other INPUT views, and `reproj_weight` x the mean over
    # the live pixels of the smallest L1 colour difference found there is added to the loss (`train_ops.photo_reprojection_loss`,
    # csrc/reproj.hip: two more launches), with gradients for the rendered depth AND alpha - the first term that hands the rasteriser
    # a `g_alpha`.  It needs no depth prior; its evidence is the other photographs.  `reproj_cameras`: which TARGET cameras carry the
    # term - "train" (the input views), "pseudo" or "all"; sources are always input views (`getTrainCameras()`) of the target's H, W
    # whose viewing direction is within `reproj_max_angle` degrees of the target's, the nearest by camera-centre distance first (ties
    # in list order); a target without one skips the term (`gs/reproj.py`).  A pixel is dead below `reproj_alpha_min`.  The term
    # starts at iteration `reproj_from_iter`.  Weighted by `reproj_weight` alone, not by the camera confidence or its map, and it
    # compares the RAW images: the exposure transform does not touch it.  The minimum over sources and the L1 form are RECALLED from
    # Monodepth2, which is not available to check against; no SSIM part, no auto-mask (cameras are posed, the scene is static),
    # alpha_min = 0.5 and the source rule are this project's choices: UNPINNED.  Out of scope: a gradient through the relative views (how q depends on
    # the poses), exposure compensation between input views, an occlusion test against a second render.  Weight 0 = off: every render,
    # gradient, launch, checkpoint file and decision is what it was.  Nothing of it goes into checkpoints.
    reproj_weight: float = 0.0
    reproj_sources: int = 2                     # 1 .. 4; chosen, UNPINNED
    reproj_cameras: str = "train"
    reproj_alpha_min: float = 0.5               # chosen, UNPINNED
    reproj_max_angle: float = 45.0              # degrees; chosen, UNPINNED
    reproj_from_iter: int = 0
    # adaptive density control, published 3DGS defaults (Kerbl et al. 2023 section 5.2 and its released arguments); used when
    # training()/finetune() run with disable_densification=False
    percent_dense: float = 0.01
    densify_from_iter: int = 500
    densify_until_iter: int = 15_000
    densification_interval: int = 100
    opacity_reset_interval: int = 3000
    densify_grad_threshold: float = 0.0002
    prune_min_opacity: float = 0.005
    prune_screen_size: float = 20.0
    # FSGS' proximity-guided Gaussian unpooling (GSTrainer.proximity_unpool; the reference's --use_proximity_densify): off by default.
    # Until iteration 2000, score > 5 x extent, scale > 1 x extent: RECALLED from FSGS' gaussian_model.py, which is not available
    # to check against - UNPINNED, and scene-scale dependent: set the factors for the scene at hand.
    use_proximity_densify: bool = False
    proximity_until_iter: int = 2000
    proximity_dist_factor: float = 5.0
    proximity_scale_factor: float = 1.0
    # Three rules of the published 3DGS optimiser (Kerbl et al. 2023 and its released training loop), all OFF by default: the
    # log-linear position learning-rate decay (`expon_lr`, `GSTrainer.update_learning_rate`), f_rest at feature_lr / div
    # (`GSTrainer.reset_optimizers`) and the progressive SH degree (`GaussianModel.oneupSHdegree`).  The released values - decay
    # 1.6e-4 -> 1.6e-6 over 30 000 steps, div 20, one degree every 1000 iterations - are RECALLED from the released 3DGS arguments,
    # which are not available to check against, and FSGS' fork may differ: UNPINNED, hence options (launch.py --gs_schedule published).
    position_lr_final: Optional[float] = None   # None: position_lr stays constant
    position_lr_delay_mult: float = 0.01
    position_lr_delay_steps: int = 0
    position_lr_max_steps: int = 30_000
    spatial_lr_scale: Optional[float] = 1.0     # multiplier of the position rate; None: cameras_extent() when the optimiser is (re)built
    feature_rest_lr_div: float = 1.0            # 1: one rate for all SH coefficients; else rows 1.. of a Gaussian at feature_lr / div
    sh_degree_interval: int = 0                 # 0: active_sh_degree stays; else oneupSHdegree() every that many iterations
    # Anti-aliased splatting (`GaussianRasterizationSettings.antialiasing`: the published 3DGS switch, Mip-Splatting's 2D Mip filter;
    # constants UNPINNED, FSGS' fork not known to have it - off by default).  A RENDERING MODE of this trainer: every render it makes
    # (train steps on both paths, `render_view` and with it `evaluate`, the capacity-seeding renders and the orchestrator's
    # render_GS) uses it.  It is NOT stored in checkpoints: a model trained with the filter has to be rendered with it (its
    # opacities have grown to make up for rho < 1), so pass the option again when a checkpoint is loaded.  Density control,
    # `reset_opacity` and pruning keep reading the raw opacity, as the published code does.
    antialiasing: bool = False
    # Mip-Splatting's 3D smoothing filter (Yu et al., CVPR 2024, section 4.1; syn3r_filter3d_compute / syn3r_raster_preprocess_f3d in
    # include/syn3r_hip.h), the other half of the method: every Gaussian is rendered with scales sqrt(s^2 + f^2) and its opacity
    # times prod s / sqrt(s^2 + f^2), f = sqrt(filter_3d_variance) / (its largest sampling rate fx / z over the training cameras that
    # see it), so no Gaussian is finer than what a training view could resolve and a render from CLOSER shows no needles or holes.
    # `GSTrainer.ensure_filter_3D` keeps `GaussianModel.filter_3D` current (every `filter_3d_interval` steps - positions move - and
    # whenever the set of Gaussians or the camera list changes); every render of the trainer passes it, a view that is not a training
    # camera does NOT recompute it.  Variance 0.2 and the interval 100 are RECALLED from the released code: UNPINNED; FSGS' fork is
    # not known to have the filter - off by default.  Density control (clone / split / prune, `reset_opacity`) keeps reading the
    # PLAIN scales and opacity, the decision taken for `antialiasing`; the released Mip-Splatting reads the filtered ones there and
    # has its own `reset_opacity`: UNPINNED, out of scope.  Unlike `antialiasing` the filter IS stored in checkpoints.
    filter_3d: bool = False
    filter_3d_variance: float = 0.2
    filter_3d_interval: int = 100
    # AbsGS' density control (Ye et al. 2024, section 3.2; gsplat's `absgrad`): the rasteriser also returns, per Gaussian, the sum over
    # its pixels of the ABSOLUTE per-pixel screen-space gradient (`rasterize_backward(abs_grad_out=)`), in which the pulls of the
    # pixels on either side of a large Gaussian over a detailed region do not cancel, and `densify_and_prune` takes the SPLIT decision
    # on its accumulated norm against `densify_abs_grad_threshold`; the CLONE decision stays on the plain gradient against
    # `densify_grad_threshold`.  Off by default: every gradient and decision is then what it was.  The threshold 0.0008 is RECALLED
    # from AbsGS' and gsplat's advice (four times the plain one), which are not available to check against: UNPINNED, and scene
    # dependent - the absolute statistic is 2 to 4 times the plain one on the test scenes, not a fixed multiple.  Not in checkpoints
    # (the statistics are not stored either).
    densify_abs_grad: bool = False
    densify_abs_grad_threshold: float = 0.0008
    # Camera-pose refinement (EXTENSION: the reference has none; what a user of InstantSplat / gsplat's `pose_opt` / MonoGS expects of a
    # sparse-view trainer whose input poses are estimates and whose pseudo-views sit at interpolated poses).  The rasteriser also
    # returns the gradient with respect to the camera (`rasterize_backward(camera_grad_out=)`), the trainer sums it per camera on the
    # device and every `pose_opt_interval` iterations (from `pose_opt_from_iter` on) takes one Adam step per camera that was
    # trained meanwhile, on the 6-vector of a left perturbation of its world-to-camera matrix (`gs/pose.py`; `GSTrainer.
    # apply_pose_updates`: ONE host read per update, none in a step).  `pose_opt_cameras`: "train" (the input views), "pseudo"
    # (the views `update_cameras` registered) or "all".  The FIRST training camera never moves: it fixes the world frame (gauge).
    # `pose_lr_rotation` is in radians; `pose_lr_translation` is multiplied by the trainer's `spatial_lr_scale` (the camera extent
    # when `spatial_lr_scale` is None).  The two rates and the interval are CHOSEN, not taken from any source: UNPINNED and scene
    # dependent.  Off by default: no table, no other rasteriser entry, every render, gradient and decision is what it was.  Refined
    # poses and their Adam state ARE stored in checkpoints (written only with the option on).  `evaluate` renders the cameras it
    # is given at THEIR poses: held-out views are not aligned to the refined frame.
    pose_opt: bool = False
    pose_opt_cameras: str = "all"
    pose_lr_rotation: float = 1e-3
    pose_lr_translation: float = 1e-3
    pose_opt_interval: int = 10
    pose_opt_from_iter: int = 0
    # Per-camera affine exposure compensation (EXTENSION: the reference has none; what a user of the published 3DGS code base's
    # per-image exposure model or of gsplat's appearance optimisation expects of a trainer that refines against generated frames,
    # whose brightness, white balance and contrast drift).  An eligible camera holds A (3 x 4, initialised to [I | 0]) and its loss
    # compares E(render), E_c = A[c][0] I_0 + A[c][1] I_1 + A[c][2] I_2 + A[c][3], with the camera's target: the photometric term (L1,
    # D-SSIM, with or without `confidence_map`) and the LPIPS term see E(render); the depth-correlation term, `render_view`,
    # `evaluate`, the capacity-seeding renders and the orchestrator's render_GS see the scene colour (`gs/exposure.py`,
    # csrc/exposure.hip; four more launches per step on an eligible camera, no host read).  `exposure_cameras`: "pseudo" (the views
    # `update_cameras` registered), "train" (the input views) or "all"; for "train" and "all" the FIRST training camera keeps the
    # identity forever (gauge: otherwise a global colour change is free).  A takes one Adam step (betas 0.9 / 0.999, eps 1e-15) per
    # step on its camera at `exposure_lr`, constant unless `exposure_lr_final` is set: then expon_lr(iteration + 1, exposure_lr,
    # exposure_lr_final, max_steps=exposure_lr_max_steps).  Rate 0.01 (to 0.001 over 30 000 steps in the released arguments) and the
    # Adam constants are RECALLED from the released 3DGS arguments, which are not available to check against: UNPINNED and scene
    # dependent.  Off by default: every render, gradient, launch, checkpoint file and decision is what it was.  A and its Adam state
    # ARE stored in checkpoints (written only with the option on).  No regulariser on A, no exposure for held-out cameras.
    exposure_opt: bool = False
    exposure_cameras: str = "pseudo"
    exposure_lr: float = 0.01
    exposure_lr_final: Optional[float] = None
    exposure_lr_max_steps: int = 30_000
    # 3DGS-MCMC density control (EXTENSION: the reference has none; Kheradmand et al., NeurIPS 2024 - what a user of gsplat's MCMC
    # strategy expects of a sparse-view trainer: no scene-dependent gradient thresholds, a budget, no opacity reset).  With `mcmc` the
    # clone / split / prune control and its opacity reset do not run; instead (`gs/mcmc.py`, csrc/mcmc.hip), every `mcmc_interval`
    # iterations inside (`densify_from_iter`, `mcmc_until_iter`), dead Gaussians (opacity <= `mcmc_min_opacity`) are relocated onto
    # live ones drawn in proportion to their opacity and N grows by 5 % towards `mcmc_cap_max`, after which N, every allocation and the
    # binning capacities stay fixed; every step adds position noise Sigma eps, gated to low-opacity Gaussians, of scale `mcmc_noise_lr`
    # x the position group's rate (0: no launch); the loss gains `mcmc_opacity_reg` x mean opacity + `mcmc_scale_reg` x mean scale, on
    # the plain opacity and scales (not the `filter_3d` ones).  No host read in a step or in a control call.  The draws are a
    # function of (`seed`, iteration, index): nothing new in checkpoints.  Not combinable with `use_proximity_densify` or
    # `densify_abs_grad`, and `mcmc_cap_max` must not be below the initial N (ValueError).  All eight values are RECALLED from the
    # paper and its released code, which are not available to check against: UNPINNED; the step on which the control runs skips the
    # optimiser step (the trainer's rule; the paper's loop does not): UNPINNED.  Off by default: every render, gradient, launch,
    # checkpoint file and decision is what it was.
    mcmc: bool = False
    mcmc_cap_max: int = 200_000                 # recalled, UNPINNED (scene dependent: the released configurations set it per scene)
    mcmc_noise_lr: float = 5e5                  # recalled, UNPINNED
    mcmc_opacity_reg: float = 0.01              # recalled, UNPINNED
    mcmc_scale_reg: float = 0.01                # recalled, UNPINNED
    mcmc_interval: int = 100                    # recalled, UNPINNED
    mcmc_until_iter: int = 25_000               # recalled, UNPINNED
    mcmc_min_opacity: float = 0.005             # recalled, UNPINNED


def expon_lr(step, lr_init: float, lr_final: float, lr_delay_steps: int = 0, lr_delay_mult: float = 1.0,
             max_steps: int = 1_000_000) -> float:
    """The published 3DGS `get_expon_lr_func` helper (general_utils; from Plenoxels / JaxNeRF) at one step, in float64:
    log-linear interpolation lr_init -> lr_final over `max_steps` (clamped beyond), times the delay factor
    lr_delay_mult + (1 - lr_delay_mult) sin(pi/2 clip(step / lr_delay_steps, 0, 1)) when lr_delay_steps > 0.
    0.0 for a negative step or when both rates are zero.  At the two ends (t = 0, t = 1) the rate is lr_init / lr_final itself, not
    exp(log(.)) of it (which may be an ulp or two away)."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    if lr_init <= 0.0 or lr_final <= 0.0:
        raise ValueError(f"expon_lr: rates must be positive (or both zero), got {lr_init} -> {lr_final}")
    delay = 1.0
    if lr_delay_steps > 0:
        delay = lr_delay_mult + (1.0 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
    t = min(max(step / max_steps, 0.0), 1.0)
    if t == 0.0 or t == 1.0:
        return delay * float(lr_init if t == 0.0 else lr_final)
    return delay * math.exp(math.log(lr_init) * (1.0 - t) + math.log(lr_final) * t)
