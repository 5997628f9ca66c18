"""Scene-parallel launcher: `DiffusionGS(...).run(refine_cycle_num)` once per scene, one process per GPU, ONE RCCL
all-gather of the per-scene record at the end.

Replaces the reference's sequential bash loop over scenes (`bash_scripts/batch_llff_train.sh:24-47`, one
`python scripts/train.py ...` after the other on a single GPU) and keeps `scripts/train.py`'s hot-path flags
(`:28-69`: --diffusion_type, --interp_type, --cam_confidence, --pseudo_cam_sampling_rate, --densify_type,
--refine_cycle_num, --num_views_for_pcd_densification, --fps_keyframe_sampling, --checkpoint_iterations, --dataset).

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m syn3r_amd.launch \\
        --scenes fern,flower,fortress,horns,leaves,orchids,room,trex --scene-factory mypkg.llff:open_scene ...

Rank r takes scenes r, r + world, ... (`dist.assign_scenes`); there is no data-path collective.  What a "scene" is
comes from a factory `f(name, args, device) -> dict(trainer=GSTrainer, num_input_views=int, test_cameras=[Camera],
svd_components=dict|None)`: dataset IO (COLMAP / LLFF readers) is outside this repository's scope, so the built-in
factory is the seeded synthetic scene the tests use (`synthetic:<seed>`), with stand-in SVD modules unless a local
checkpoint directory is given (`--svd_dir`, loaded by `StableVideoDiffusionPipeline.from_pretrained`: UNet, VAE, scheduler, CLIP).
A scene that raises is recorded with NaN metrics and ok = 0; the other ranks are unaffected.
"""
from __future__ import annotations

import argparse
import importlib
import math
import os
import sys
import time
import traceback
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from . import dist as D


def parse(argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0], epilog=(
        "Accepted and ignored (flags of the absent FSGS parameter groups that the reference's batch scripts pass): "
        + " ".join(sorted(FSGS_FLAGS)) + ".  --svd_l1_weight (batch_dl3dv_train.sh:87) belongs to the absent fork too: its meaning is "
        "not visible, so it has none here."))
    ap.add_argument("--scenes", type=str, required=True, help="comma-separated scene names")
    ap.add_argument("--scene-factory", type=str, default="syn3r_amd.launch:synthetic_scene",
                    help="module:function building one scene (see the module docstring)")
    ap.add_argument("--model_path", type=str, default="output", help="per-scene artefacts go to <model_path>/<scene>")
    ap.add_argument("--svd_dir", type=str, default=None, help="local SVD checkpoint directory in the diffusers layout (unet/, vae/, scheduler/, image_encoder/, feature_extractor/)")
    ap.add_argument("--backend", type=str, default=None, help="torch.distributed backend (default: nccl = RCCL on a GPU box)")
    # scripts/train.py:28-69, flag for flag with the reference's defaults and choices (tests/golden/train_flags.json, captured
    # from the script by oracle/gen_golden.py train_flags; tests/test_dist_cpu.py compares).  As in the reference the default
    # --diffusion_type '2Pass' and --densify_type 'interpolate' are not among the types the orchestrator accepts
    # (model/diffusionGS.py:115-124, :244-255 raise NotImplementedError): the batch scripts always pass both.
    ap.add_argument("--major_radius", type=float, default=50)           # parsed, unused by the live path
    ap.add_argument("--minor_radius", type=float, default=40)
    ap.add_argument("--weight_clamp", type=float, default=0.4)
    ap.add_argument("--image_path", type=str)
    ap.add_argument("--folder_path", type=str)
    ap.add_argument("--iteration", type=str)
    ap.add_argument("--inverse", type=bool, default=False)
    ap.add_argument("--degrees_per_frame", type=float, default=0.4)
    ap.add_argument("--ip", type=str, default="127.0.0.1")
    ap.add_argument("--port", type=int, default=6007)
    ap.add_argument("--debug_from", type=int, default=-100)
    ap.add_argument("--detect_anomaly", action="store_true", default=False)
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--start_checkpoint", type=str, default=None)
    ap.add_argument("--diffusion_type", type=str, default="2Pass")
    ap.add_argument("--interp_type", type=str, default="forward_warp", choices=["forward_warp", "backward_warp"])
    ap.add_argument("--near", type=int, default=0)
    ap.add_argument("--cam_confidence", type=float, default=0.1)
    ap.add_argument("--pseudo_cam_sampling_rate", type=float, default=0.04)
    ap.add_argument("--test_iterations", nargs="+", type=int, default=[5_000, 10_000])
    ap.add_argument("--save_iterations", nargs="+", type=int, default=[5_000, 10_000])
    ap.add_argument("--checkpoint_iterations", nargs="+", type=int, default=[8_000, 10_000])
    ap.add_argument("--train_bg", action="store_true")
    ap.add_argument("--densify_type", type=str, default="interpolate",
                    choices=["interpolate", "from_single", "from_single_gs", "interpolate_gs", "interpolate_loop0_gs", "interpolate_gs_v2"])
    ap.add_argument("--dataset", type=str, default="llff", choices=["llff", "dtu", "dl3dv"])
    ap.add_argument("--refine_cycle_num", type=int, default=1)
    ap.add_argument("--reorg_train_views", type=int, default=1)
    ap.add_argument("--num_views_for_pcd_densification", type=int, default=4)
    ap.add_argument("--fps_keyframe_sampling", type=int, default=0, help="If >0, use FPS for keyframe selection during PCD densification")
    # the trainer's own parameters (FSGS' ModelParams / OptimizationParams groups are absent: the ones this trainer reads)
    ap.add_argument("--iterations", type=int, default=10_000)
    ap.add_argument("--lambda_dssim", type=float, default=0.2)
    ap.add_argument("--lpips_weight", type=float, default=0.0,
                    help="weight of the LPIPS term during refines (bash_scripts/batch_dl3dv_train.sh:84-87 passes 1); needs --lpips_weights")
    ap.add_argument("--lpips_weights", type=str, default=None,
                    help="local state_dict file of lpips.LPIPS(net='vgg') (torch.save format); the package's download is not reachable offline")
    ap.add_argument("--lpips_precision", type=str, default="fp16", choices=("fp16", "fp16x2"),
                    help="activation storage of the LPIPS model built from --lpips_weights: fp16 (default), or fp16x2 = every forward "
                         "activation as an fp16 pair hi + lo (image gradient 5e-4 .. 9e-4 instead of 5-6 %% away from float64; the "
                         "forward convolutions of the render double their K; gs/lpips.py)")
    ap.add_argument("--depth_weight", type=float, default=0.0,
                    help="weight of FSGS' depth-correlation term, 1 - Pearson(rendered depth, monocular prior), on every training step "
                         "(0 = off); views need a prior (Camera.depth_image or an injected GSTrainer.depth_net)")
    ap.add_argument("--depth_local_weight", type=float, default=0.0,
                    help="EXTENSION (not in the reference): weight of the PATCH-WISE depth-correlation term, the mean over "
                         "--depth_patch_size pixel patches of 1 - Pearson(rendered depth, prior) per patch (a monocular prior is "
                         "consistent only locally), next to --depth_weight (0 = off); the patch grid's origin is drawn per step")
    ap.add_argument("--depth_patch_size", type=int, default=32,
                    help="patch size of --depth_local_weight in pixels (2 .. 256, no larger than a view's sides); chosen, not taken "
                         "from a source, and resolution dependent")
    ap.add_argument("--depth_smooth_weight", type=float, default=0.0,
                    help="EXTENSION (not in the reference): weight of the prior-free edge-aware smoothness term on the rendered depth, "
                         "(S_x + S_y) / mean depth with S the mean of exp(-gamma |image gradient|) |depth gradient| per direction "
                         "(Monodepth2's form; needs no depth prior, so it runs on pseudo-views as well); 0 = off")
    ap.add_argument("--depth_smooth_gamma", type=float, default=1.0,
                    help="OptimizationParams.depth_smooth_gamma: the edge weights' decay with the target image's contrast (1: "
                         "recalled from Monodepth2, UNPINNED)")
    ap.add_argument("--depth_smooth_cameras", type=str, default="all", choices=("all", "train", "pseudo"),
                    help="OptimizationParams.depth_smooth_cameras: the cameras --depth_smooth_weight acts on - the input views, the "
                         "diffusion pseudo-views, or both")
    ap.add_argument("--reproj_weight", type=float, default=0.0,
                    help="EXTENSION (not in the reference): weight of the multi-view photometric reprojection term - the rendered depth "
                         "carries each pixel into other input views and the smallest L1 colour difference found there is penalised "
                         "(Monodepth2's minimum reprojection error, no SSIM, no auto-mask; gradients for depth and alpha); 0 = off")
    ap.add_argument("--reproj_sources", type=int, default=2, choices=(1, 2, 3, 4),
                    help="OptimizationParams.reproj_sources: source views per target, the nearest input views first")
    ap.add_argument("--reproj_cameras", type=str, default="train", choices=("train", "pseudo", "all"),
                    help="OptimizationParams.reproj_cameras: the TARGET cameras --reproj_weight acts on - the input views, the diffusion "
                         "pseudo-views, or both; sources are always input views")
    ap.add_argument("--reproj_alpha_min", type=float, default=0.5,
                    help="OptimizationParams.reproj_alpha_min: a pixel below this rendered alpha is left out (chosen, UNPINNED)")
    ap.add_argument("--reproj_max_angle", type=float, default=45.0,
                    help="OptimizationParams.reproj_max_angle: largest angle in degrees between the viewing directions of a target and "
                         "a source (chosen, UNPINNED)")
    ap.add_argument("--reproj_from_iter", type=int, default=0,
                    help="OptimizationParams.reproj_from_iter: first iteration that carries the term")
    ap.add_argument("--pixel_confidence", type=int, default=0, choices=(0, 1),
                    help="1: EXTENSION (not in the reference) - every diffusion pseudo-view is weighted per pixel in the photometric loss by "
                         "1 - the fused uncertainty of its interpolation (backward_warp only), on top of --cam_confidence; the pairs' .pt "
                         "caches gain a `confidence_maps` key.  0 (default): the reference's scalar weight alone")
    ap.add_argument("--use_proximity_densify", type=int, default=0,
                    help="1: FSGS' proximity-guided Gaussian unpooling inside the density control (bash_scripts/batch_llff_train.sh:37 and "
                         "batch_dl3dv_train.sh:85 pass 0); thresholds: OptimizationParams.proximity_*")
    # FSGS' OptimizationParams / ModelParams flags that this trainer has a field for (bash_scripts/batch_llff_train.sh:37 and
    # batch_dl3dv_train.sh:85 pass --densify_grad_threshold 0.0002 --percent_dense 0.001).  None = leave OptimizationParams alone.
    for flag, typ in TRAINER_FLAGS:
        ap.add_argument("--" + flag, type=typ, default=None,
                        help=f"OptimizationParams.{TRAINER_FLAG_FIELDS.get(flag, flag)} (default: the trainer's own)" if flag != "sh_degree"
                        else "largest SH degree of the model the scene factory builds (default: the factory's own)")
    ap.add_argument("--gs_schedule", type=str, default="constant", choices=("constant", "published"),
                    help="published: the three rules of the published 3DGS optimiser - position rate decaying log-linearly to "
                         "--position_lr_final (default 1.6e-6) over --position_lr_max_steps, times the camera extent; SH rows 1.. at "
                         "feature_lr / 20; SH degree from 0, one up every 1000 iterations (values recalled, UNPINNED: "
                         "gs/params.py OptimizationParams).  constant (default): none of them")
    ap.add_argument("--antialiasing", type=int, default=0, choices=(0, 1),
                    help="1: anti-aliased splatting in every render of the trainer (OptimizationParams.antialiasing: the published 3DGS "
                         "switch = Mip-Splatting's 2D Mip filter; constants recalled, UNPINNED).  Not stored in checkpoints: a model "
                         "trained with it has to be rendered with it.  0 (default): the plain 0.3 px dilation")
    ap.add_argument("--filter_3d", type=int, default=0, choices=(0, 1),
                    help="1: Mip-Splatting's 3D smoothing filter in every render of the trainer (OptimizationParams.filter_3d: every "
                         "Gaussian bounded from below by the sampling rate of the training cameras; constants recalled, UNPINNED).  "
                         "The filter is stored in checkpoints.  0 (default): off")
    ap.add_argument("--densify_abs_grad", type=int, default=0, choices=(0, 1),
                    help="1: AbsGS' density control (OptimizationParams.densify_abs_grad): the split decision is taken on the "
                         "accumulated ABSOLUTE screen-space gradient against --densify_abs_grad_threshold, the clone decision stays "
                         "on the plain one against --densify_grad_threshold.  0 (default): the published 3DGS rule for both")
    ap.add_argument("--densify_abs_grad_threshold", type=float, default=None,
                    help="OptimizationParams.densify_abs_grad_threshold (default: the trainer's own, 0.0008 - recalled, UNPINNED, "
                         "scene dependent)")
    ap.add_argument("--pose_opt", type=int, default=0, choices=(0, 1),
                    help="1: EXTENSION (not in the reference) - camera-pose refinement (OptimizationParams.pose_opt): the rasteriser also "
                         "returns the gradient with respect to the camera and the trainer takes an Adam step on the poses of "
                         "--pose_opt_cameras every --pose_opt_interval iterations; the first training camera stays fixed.  evaluate() "
                         "does not align held-out poses to the refined frame.  0 (default): cameras never move")
    ap.add_argument("--pose_opt_cameras", type=str, default=None, choices=("train", "pseudo", "all"),
                    help="OptimizationParams.pose_opt_cameras: the input views, the diffusion pseudo-views, or both (default: the trainer's own, all)")
    ap.add_argument("--pose_lr_rotation", type=float, default=None,
                    help="OptimizationParams.pose_lr_rotation, radians (default: the trainer's own, 1e-3 - chosen, UNPINNED, scene dependent)")
    ap.add_argument("--pose_lr_translation", type=float, default=None,
                    help="OptimizationParams.pose_lr_translation, times the spatial scale (default: the trainer's own, 1e-3 - chosen, UNPINNED)")
    ap.add_argument("--pose_opt_interval", type=int, default=None,
                    help="OptimizationParams.pose_opt_interval: iterations between pose updates (default: the trainer's own, 10 - chosen, UNPINNED)")
    ap.add_argument("--exposure_opt", type=int, default=0, choices=(0, 1),
                    help="1: EXTENSION (not in the reference) - per-camera affine exposure compensation (OptimizationParams.exposure_opt): "
                         "a camera of --exposure_cameras holds a 3 x 4 colour transform between its render and the photometric / LPIPS "
                         "terms, with an Adam step of its own per step on that camera; the first training camera keeps the identity.  "
                         "Renders, evaluate() and the depth term keep the scene colour.  0 (default): no camera has one")
    ap.add_argument("--exposure_cameras", type=str, default=None, choices=("pseudo", "train", "all"),
                    help="OptimizationParams.exposure_cameras: the diffusion pseudo-views, the input views, or both (default: the "
                         "trainer's own, pseudo)")
    ap.add_argument("--exposure_lr", type=float, default=None,
                    help="OptimizationParams.exposure_lr (default: the trainer's own, 0.01 - recalled, UNPINNED, scene dependent)")
    ap.add_argument("--exposure_lr_final", type=float, default=None,
                    help="OptimizationParams.exposure_lr_final: the rate decays log-linearly to it over exposure_lr_max_steps (default: "
                         "the trainer's own, None = constant)")
    ap.add_argument("--mcmc", type=int, default=0, choices=(0, 1),
                    help="1: EXTENSION (not in the reference) - 3DGS-MCMC density control (OptimizationParams.mcmc): dead Gaussians are "
                         "relocated onto live ones, N grows 5 %% per call to --mcmc_cap_max and then stays, position noise every step, L1 "
                         "regularisers on opacity and scale; no clone / split / prune, no opacity reset.  Not with "
                         "--use_proximity_densify or --densify_abs_grad.  0 (default): the published control")
    ap.add_argument("--mcmc_cap_max", type=int, default=None,
                    help="OptimizationParams.mcmc_cap_max: the budget of Gaussians (default: the trainer's own, 200000 - recalled, UNPINNED)")
    ap.add_argument("--mcmc_noise_lr", type=float, default=None,
                    help="OptimizationParams.mcmc_noise_lr: noise scale over the position rate, 0 = no noise (default: the trainer's own, "
                         "5e5 - recalled, UNPINNED)")
    ap.add_argument("--mcmc_opacity_reg", type=float, default=None,
                    help="OptimizationParams.mcmc_opacity_reg (default: the trainer's own, 0.01 - recalled, UNPINNED)")
    ap.add_argument("--mcmc_scale_reg", type=float, default=None,
                    help="OptimizationParams.mcmc_scale_reg (default: the trainer's own, 0.01 - recalled, UNPINNED)")
    ap.add_argument("--num_inference_steps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    # FSGS' parameter groups (scripts/train.py:44-46: -s, --eval, --n_views, --resolution, --use_dust3r ... of the batch scripts)
    # belong to the absent submodule: a command line that carries them is accepted, they are kept in `ignored_flags`
    given = list(sys.argv[1:] if argv is None else argv)
    args, rest = ap.parse_known_args(given)
    # argparse takes `--percent_dens` for an abbreviation of `--percent_dense`: while that flag sat in FSGS_FLAGS the token was an
    # unknown argument, and a misspelling stays one
    declared = ["--" + f for f, _ in TRAINER_FLAGS] + ["--gs_schedule", "--pixel_confidence", "--antialiasing", "--filter_3d",
                                                       "--densify_abs_grad", "--densify_abs_grad_threshold", "--pose_opt",
                                                       "--pose_opt_cameras", "--pose_lr_rotation", "--pose_lr_translation",
                                                       "--pose_opt_interval", "--exposure_opt", "--exposure_cameras", "--exposure_lr",
                                                       "--exposure_lr_final", "--mcmc", "--mcmc_cap_max", "--mcmc_noise_lr",
                                                       "--mcmc_opacity_reg", "--mcmc_scale_reg", "--depth_smooth_weight",
                                                       "--depth_smooth_gamma", "--depth_smooth_cameras", "--reproj_weight",
                                                       "--reproj_sources", "--reproj_cameras", "--reproj_alpha_min",
                                                       "--reproj_max_angle", "--reproj_from_iter"]
    # (a token that IS a declared flag is not an abbreviation of a longer one: --densify_abs_grad / --densify_abs_grad_threshold)
    cut = [t for t in given if t.startswith("--") and t.split("=")[0] not in declared
           and any(d.startswith(t.split("=")[0]) for d in declared)]
    if cut:
        ap.error(f"unknown argument(s): {' '.join(cut)} (the trainer's flags are not abbreviated)")
    # Only the flags of FSGS' ModelParams / OptimizationParams / PipelineParams groups that the reference's batch scripts pass
    # (bash_scripts/*.sh) are tolerated; anything else is a misspelling of one of ours and an error - a dropped
    # `--iteratons 500` must not start a multi-hour job on the defaults.
    unknown = [t for t in rest if t.startswith("-") and not _is_number(t) and t not in FSGS_FLAGS]
    if unknown:
        ap.error(f"unknown argument(s): {' '.join(unknown)} (flags of the FSGS parameter groups that are accepted and ignored: "
                 f"{' '.join(sorted(FSGS_FLAGS))})")
    args.ignored_flags = list(rest)
    return args


# FSGS' optimiser / model flags with a counterpart in this trainer (published 3DGS OptimizationParams / ModelParams names), and the
# OptimizationParams field of those whose name differs
TRAINER_FLAGS = (
    ("percent_dense", float), ("densify_grad_threshold", float), ("densify_from_iter", int), ("densify_until_iter", int),
    ("densification_interval", int), ("opacity_reset_interval", int), ("position_lr_init", float), ("position_lr_final", float),
    ("position_lr_max_steps", int), ("feature_lr", float), ("opacity_lr", float), ("scaling_lr", float), ("rotation_lr", float),
    ("sh_degree", int))
TRAINER_FLAG_FIELDS = {"position_lr_init": "position_lr"}


def apply_trainer_flags(opt, args):
    """-> a copy of `opt` (gs.OptimizationParams) with the TRAINER_FLAGS that were given (not None) in their fields, and with
    `--gs_schedule published` the switches of the three published optimiser rules: decay to --position_lr_final or 1.6e-6,
    spatial_lr_scale = None (the camera extent), feature_rest_lr_div = 20, sh_degree_interval = 1000.  Pure: no GPU, `opt`
    untouched.  `--antialiasing 1` sets `antialiasing`, `--filter_3d 1` sets `filter_3d`, `--densify_abs_grad 1` sets `densify_abs_grad`
    (0, the default, leaves the field as `opt` has it); `--densify_abs_grad_threshold`, when given, sets its field.  `--pose_opt 1`
    sets `pose_opt`; `--pose_opt_cameras`, `--pose_lr_rotation`, `--pose_lr_translation` and `--pose_opt_interval`, when given, set theirs.
    `--exposure_opt 1` sets `exposure_opt`; `--exposure_cameras`, `--exposure_lr` and `--exposure_lr_final`, when given, set theirs.
    `--mcmc 1` sets `mcmc`; `--mcmc_cap_max`, `--mcmc_noise_lr`, `--mcmc_opacity_reg` and `--mcmc_scale_reg`, when given, set theirs.
    `--depth_smooth_weight`, `--depth_smooth_gamma` and `--depth_smooth_cameras` set theirs (the flags' defaults are the options' own: 0, 1, "all").
    `--reproj_weight`, `--reproj_sources`, `--reproj_cameras`, `--reproj_alpha_min`, `--reproj_max_angle` and `--reproj_from_iter` set
    theirs likewise (defaults 0, 2, "train", 0.5, 45, 0); a value the term cannot run with is a ValueError (`gs.reproj.check_options`).  (--sh_degree
    describes the model, not the optimiser: the scene factory reads it.)"""
    import dataclasses
    new = {}
    for flag, _ in TRAINER_FLAGS:
        v = getattr(args, flag, None)
        if v is not None and flag != "sh_degree":
            new[TRAINER_FLAG_FIELDS.get(flag, flag)] = v
    if getattr(args, "gs_schedule", "constant") == "published":
        if new.get("position_lr_final", opt.position_lr_final) is None:
            new["position_lr_final"] = 1.6e-6
        new.update(spatial_lr_scale=None, feature_rest_lr_div=20.0, sh_degree_interval=1000)
    if getattr(args, "antialiasing", 0):
        new["antialiasing"] = True
    if getattr(args, "filter_3d", 0):
        new["filter_3d"] = True
    if getattr(args, "densify_abs_grad", 0):
        new["densify_abs_grad"] = True
    if getattr(args, "densify_abs_grad_threshold", None) is not None:
        new["densify_abs_grad_threshold"] = float(args.densify_abs_grad_threshold)
    if getattr(args, "pose_opt", 0):
        new["pose_opt"] = True
    for flag, typ in (("pose_opt_cameras", str), ("pose_lr_rotation", float), ("pose_lr_translation", float), ("pose_opt_interval", int)):
        if getattr(args, flag, None) is not None:
            new[flag] = typ(getattr(args, flag))
    if getattr(args, "exposure_opt", 0):
        new["exposure_opt"] = True
    for flag, typ in (("exposure_cameras", str), ("exposure_lr", float), ("exposure_lr_final", float)):
        if getattr(args, flag, None) is not None:
            new[flag] = typ(getattr(args, flag))
    if getattr(args, "mcmc", 0):
        new["mcmc"] = True
    for flag, typ in (("mcmc_cap_max", int), ("mcmc_noise_lr", float), ("mcmc_opacity_reg", float), ("mcmc_scale_reg", float)):
        if getattr(args, flag, None) is not None:
            new[flag] = typ(getattr(args, flag))
    for flag, typ in (("depth_smooth_weight", float), ("depth_smooth_gamma", float), ("depth_smooth_cameras", str)):
        if getattr(args, flag, None) is not None:
            new[flag] = typ(getattr(args, flag))
    for flag, typ in (("reproj_weight", float), ("reproj_sources", int), ("reproj_cameras", str), ("reproj_alpha_min", float),
                      ("reproj_max_angle", float), ("reproj_from_iter", int)):
        if getattr(args, flag, None) is not None:
            new[flag] = typ(getattr(args, flag))
    out = dataclasses.replace(opt, **new)
    from .gs.reproj import check_options
    check_options(out)
    return out


# scripts/train.py:44-46 builds FSGS' three parameter groups on the parser; these are the flags of theirs that the reference's
# bash_scripts/batch_{llff,dtu,dl3dv}_train.sh pass on the command line and that nothing here reads.  --svd_l1_weight
# (batch_dl3dv_train.sh:87) belongs to the absent fork as well: its meaning is not visible, so it is accepted and ignored.
FSGS_FLAGS = frozenset([
    "-s", "--source_path", "-m", "-r", "--resolution", "--images", "-i", "--eval", "--n_views", "--use_dust3r", "--rand_pcd",
    "--num_train_samples", "--sample_pseudo_interval", "--sample_svd_pseudo_interval", "--start_sample_svd_frame",
    "--start_sample_pseudo", "--end_sample_pseudo", "--svd_depth_warmup", "--svd_lpips_weight", "--svd_l1_weight",
    "--depth_pseudo_weight", "--white_background",
    "--data_device", "--convert_SHs_python", "--compute_cov3D_python", "--debug", "--checkpoint", "--video", "-a", "-p", "-f", "-d",
])
# the types the orchestrator accepts (model/diffusionGS.py:115-124, :244-255; syn3r_amd/diffusionGS.py raises on the rest)
DIFFUSION_TYPES = ("2PassProbUncertain", "2PassProbUncertainPost")
DENSIFY_TYPES = ("interpolate_loop0_gs", "interpolate_gs_v2")


def _is_number(t: str) -> bool:
    try:
        float(t)
        return True
    except ValueError:
        return False


def validate(args) -> None:
    """What `parse` cannot reject without departing from the reference's parser (whose DEFAULTS, '2Pass' / 'interpolate', are
    types its own orchestrator refuses): checked by `main` before any GPU work, so a bad command line exits non-zero instead
    of producing one NaN record per scene."""
    if args.diffusion_type not in DIFFUSION_TYPES:              # (DiffusionGS.__init__ raises on it whatever the cycle count)
        raise SystemExit(f"--diffusion_type {args.diffusion_type!r} is not accepted by the orchestrator (model/diffusionGS.py:115-124): "
                         f"pass one of {', '.join(DIFFUSION_TYPES)}")
    if args.refine_cycle_num > 0 and args.densify_type not in DENSIFY_TYPES:
        raise SystemExit(f"--densify_type {args.densify_type!r} is not accepted by the orchestrator (model/diffusionGS.py:244-255): "
                         f"pass one of {', '.join(DENSIFY_TYPES)}")


def synthetic_scene(name: str, args, device) -> dict:
    """`synthetic:<seed>[:<N>]` — a seeded Gaussian cloud rendered from three cameras on a baseline (the views to fit),
    a perturbed copy of it as the initial model, and two held-out cameras between the inputs for PSNR / SSIM.  Each training
    camera carries the truth cloud's disparity as its depth prior (`depth_image`: alpha / depth where alpha >= 0.5, else 0;
    read only when `--depth_weight` or `--depth_local_weight` > 0).  `--sh_degree` d (0..3): the model's largest SH degree; the 16 coefficient rows stay,
    those above (d + 1)^2 are never read."""
    from .gs import Camera, GaussianModel, GSTrainer, OptimizationParams
    from .synthetic import synthetic_gaussians
    parts = name.split(":")
    seed = int(parts[1]) if len(parts) > 1 else 0
    N = int(parts[2]) if len(parts) > 2 else 2000
    H, W = 72, 128
    m, s, q, o, sh = synthetic_gaussians(N, seed=seed, log_scale_mean=math.log(0.08))
    logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
    truth = GaussianModel(m, torch.log(s), q, logit, sh, device=device)
    f = W / (2 * math.tan(math.radians(30)))
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=np.float32)

    def pose(dx):
        p = np.eye(4, dtype=np.float32)
        p[0, 3] = dx
        return p

    gt = GSTrainer(truth, [Camera.from_w2c(pose(0.0), K, H, W, data_device=device)])
    shot = lambda dx: gt.render_view(Camera.from_w2c(pose(dx), K, H, W, data_device=device))["render"].detach().clamp(0, 1)
    train = [Camera.from_w2c(pose(dx), K, H, W, image=shot(dx), data_device=device,
                             depth_image=truth_disparity(gt, Camera.from_w2c(pose(dx), K, H, W, data_device=device)))
             for dx in (-0.15, 0.0, 0.15)]
    test = [Camera.from_w2c(pose(dx), K, H, W, image=shot(dx), data_device=device) for dx in (-0.075, 0.075)]
    g = torch.Generator().manual_seed(seed + 1)
    sh_degree = 3 if getattr(args, "sh_degree", None) is None else int(args.sh_degree)
    model = GaussianModel(m + 0.01 * torch.randn(m.shape, generator=g), torch.log(s), q, logit, sh, sh_degree=sh_degree, device=device)
    opt = OptimizationParams(iterations=args.iterations, lambda_dssim=args.lambda_dssim, seed=args.seed)
    out_dir = os.path.join(args.model_path, name.replace(":", "_"))
    trainer = GSTrainer(model, train, opt, model_path=out_dir, checkpoint_iterations=args.checkpoint_iterations)
    return dict(trainer=trainer, num_input_views=len(train), test_cameras=test, svd_components=None)


@torch.no_grad()
def truth_disparity(trainer, cam) -> torch.Tensor:
    """Disparity prior [H,W] of a view from the cloud a trainer holds: the inverse of the alpha-normalised rendered depth,
    alpha / depth, where the accumulated alpha is >= 0.5 and 0 elsewhere (a stand-in for a monocular network's output)."""
    out = trainer.render_view(cam)
    depth, alpha = out["depth"][0], out["alpha"][0]
    ok = (alpha >= 0.5) & (depth > 0)
    return torch.where(ok, alpha / torch.where(ok, depth, torch.ones_like(depth)), torch.zeros_like(depth)).contiguous()


def _stand_in_svd(device):
    """Deterministic stand-ins with the interfaces of CLIP / VAE / UNet for runs without a local checkpoint: the loop
    logic, the warps, the scheduler kernels and the rasteriser run for real, the networks do not."""
    class Enc:
        def __call__(self, image):
            from types import SimpleNamespace
            return SimpleNamespace(image_embeds=torch.zeros(1, 1024))

    class Vae:
        config = type("C", (), {"scaling_factor": 0.18215})()

        def encode(self, x):
            from types import SimpleNamespace
            z = torch.nn.functional.avg_pool2d(x, 8)
            z = torch.cat([z, z[:, :1]], 1)
            return SimpleNamespace(latent_dist=SimpleNamespace(mode=lambda: z))

        def decode(self, z, num_frames=1):
            from types import SimpleNamespace
            return SimpleNamespace(sample=torch.nn.functional.interpolate(z[:, :3], scale_factor=8, mode="nearest"))

    class UNet:
        def __call__(self, x, t, encoder_hidden_states=None, added_time_ids=None, return_dict=False):
            return (0.1 * x[:, :, :4],)

    return dict(vae=Vae(), image_encoder=Enc(), unet=UNet(), dtype=torch.float32)


def run_scene(name: str, args, device, factory: Callable) -> List[float]:
    """One scene end to end -> the RECORD_FIELDS record."""
    from .diffusionGS import DiffusionGS
    t0 = time.perf_counter()
    sc = factory(name, args, device)
    trainer = sc["trainer"]
    comps = sc.get("svd_components")
    if comps is None and args.refine_cycle_num > 0:
        # --svd_dir: the whole pipeline from a local diffusers-layout checkpoint (unet/, vae/, scheduler/, image_encoder/,
        # feature_extractor/), loaded by DiffusionGS.svd_render through StableVideoDiffusionPipeline.from_pretrained
        # (model/diffusionGS.py:1089); without it the plumbing stand-ins
        comps = args.svd_dir if args.svd_dir else _stand_in_svd(device)
    trainer.opt.lpips_weight = float(getattr(args, "lpips_weight", 0.0))
    trainer.opt.depth_weight = float(getattr(args, "depth_weight", 0.0))
    trainer.opt.depth_local_weight = float(getattr(args, "depth_local_weight", 0.0))
    trainer.opt.depth_patch_size = int(getattr(args, "depth_patch_size", 32))
    trainer.opt.use_proximity_densify = bool(getattr(args, "use_proximity_densify", 0))
    trainer.opt = apply_trainer_flags(trainer.opt, args)
    if getattr(args, "gs_schedule", "constant") == "published" and trainer.iteration == 0:
        trainer.gaussians.active_sh_degree = 0      # a fresh model (a factory that loaded a checkpoint has iteration > 0)
    trainer.reset_optimizers()                      # the groups' rates and the features' row split follow the flags
    if sc.get("lpips") is not None:
        trainer.lpips = sc["lpips"]
    elif getattr(args, "lpips_weights", None):
        from .gs.lpips import LPIPS
        trainer.lpips = LPIPS(precision=getattr(args, "lpips_precision", "fp16")).load_state_dict(torch.load(args.lpips_weights, map_location="cpu", weights_only=True), device)
    runner = DiffusionGS(trainer, num_input_views=sc["num_input_views"], save_dir=trainer.scene.model_path,
                         diffusion_type=args.diffusion_type, interp_type=args.interp_type, input_args=args,
                         svd_components=comps, num_inference_steps=args.num_inference_steps,
                         diffusion_size=sc.get("diffusion_size", (576, 1024)))
    it0 = trainer.iteration
    np.random.seed(args.seed)               # the orchestrator's pose perturbation draws from np.random (diffusionGS.py:653)
    runner.run(args.refine_cycle_num)
    torch.cuda.synchronize(device)
    wall = time.perf_counter() - t0
    ev = trainer.evaluate(sc.get("test_cameras"))
    iters = trainer.iteration - it0
    units = 2.0 * args.num_inference_steps * args.refine_cycle_num * max(sc["num_input_views"] - (args.densify_type == "interpolate_loop0_gs"), 0)
    if trainer.truncated_renders:
        print(f"[syn3r] scene {name}: {trainer.truncated_renders} training render(s) ran with a truncated pair list",
              file=sys.stderr, flush=True)
    return [0.0, ev["psnr"], ev["ssim"], ev["lpips"], iters / wall, units / wall, wall,
            float(trainer.truncated_renders), 1.0]


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = parse(argv)
    validate(args)
    rank, world, local = D.init(args.backend)
    if rank == 0 and args.ignored_flags:
        print(f"[syn3r] flags of the absent FSGS parameter groups ignored: {' '.join(args.ignored_flags)}", file=sys.stderr, flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("syn3r_amd.launch needs a HIP device (the SYN3R hot path has no CPU fallback)")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    mod, fn = args.scene_factory.split(":")
    factory = getattr(importlib.import_module(mod), fn)
    scenes = [s for s in args.scenes.split(",") if s]
    mine = D.assign_scenes(scenes, rank, world)
    rounds = math.ceil(len(scenes) / world)
    table = []
    for k in range(rounds):                     # a rank with no scene left contributes a NaN row (ok = 0)
        rec = [float("nan")] * len(D.RECORD_FIELDS)
        rec[-1] = 0.0
        if k < len(mine):
            try:
                rec = run_scene(mine[k], args, device, factory)
            except Exception:                   # scenes are independent: record the failure, keep the job alive
                traceback.print_exc()
                rec = [float("nan")] * len(D.RECORD_FIELDS)
                rec[-1] = 0.0
            rec[0] = float(scenes.index(mine[k]))
        table.append(rec)
    allrec = D.gather_record_table(table).cpu()          # the job's ONE collective (RCCL all-gather over xGMI)
    if rank == 0:
        allrec = allrec[~torch.isnan(allrec[:, 0])]
        allrec = allrec[allrec[:, 0].argsort()]
        print(D.summary_table(allrec))
    if world > 1:
        torch.distributed.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
