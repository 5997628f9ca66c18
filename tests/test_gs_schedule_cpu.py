"""The published 3DGS schedule's host side: `expon_lr`, the optimiser flags of the reference's batch scripts on the launcher's
parser, and their mapping onto `OptimizationParams` (`launch.apply_trainer_flags`).  No GPU."""
import dataclasses
import math

import numpy as np
import pytest


def _published(step, lr_init, lr_final, delay_steps, delay_mult, max_steps):
    """`get_expon_lr_func`'s inner helper written out in numpy float64."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    delay = np.float64(1.0)
    if delay_steps > 0:
        delay = delay_mult + (1 - delay_mult) * np.sin(0.5 * np.pi * np.clip(step / delay_steps, 0, 1))
    t = np.clip(step / max_steps, 0, 1)
    return float(delay * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t))


@pytest.mark.parametrize("delay_steps", [0, 100])
def test_expon_lr_is_the_published_helper(delay_steps):
    from syn3r_amd.gs.trainer import expon_lr
    lr_init, lr_final, mult, max_steps = 1.6e-4, 1.6e-6, 0.01, 30_000
    # the exponent is a sum of two products of |log lr| <= 13.4: log, the products, the sum and exp each round once, in an
    # exponent of magnitude < 16 (ulp 1.8e-15) and in the result (2.2e-16); two libms may differ by an ulp in each: 8 ulp(16)
    rtol = 8 * float(np.spacing(16.0))
    for step in (0, 1, max_steps // 2, max_steps, 2 * max_steps):
        got = expon_lr(step, lr_init, lr_final, delay_steps, mult, max_steps)
        assert isinstance(got, float)
        ref = _published(step, lr_init, lr_final, delay_steps, mult, max_steps)
        assert abs(got - ref) <= rtol * ref, (step, got, ref)
    if delay_steps == 0:
        assert expon_lr(0, lr_init, lr_final, 0, mult, max_steps) == lr_init
        for step in (max_steps, max_steps + 1, 2 * max_steps):
            # the issue's bound is 1 ulp of exp / log; the ends are returned as given, so the bound met is 0
            assert expon_lr(step, lr_init, lr_final, 0, mult, max_steps) == lr_final
        mid = expon_lr(max_steps // 2, lr_init, lr_final, 0, mult, max_steps)
        assert abs(mid - 1.6e-5) <= rtol * 1.6e-5                     # the geometric mean half way
    else:
        assert expon_lr(0, lr_init, lr_final, delay_steps, mult, max_steps) == mult * lr_init      # sin(0) = 0
        assert expon_lr(2 * max_steps, lr_init, lr_final, delay_steps, mult, max_steps) == lr_final
    assert expon_lr(5, 0.0, 0.0, delay_steps, mult, max_steps) == 0.0
    assert expon_lr(-1, lr_init, lr_final, delay_steps, mult, max_steps) == 0.0


# GS_args of bash_scripts/batch_llff_train.sh:36-37 (paths shortened), as the shell splits them
LLFF_GS_ARGS = ["-s", "data/llff/fern", "--model_path", "out/fern", "--eval", "--n_views", "3", "--sample_pseudo_interval",
                "100000000000000000000", "--sample_svd_pseudo_interval", "1", "--num_train_samples", "3", "--resolution", "1", "--use_proximity_densify", "0", "--densify_grad_threshold", "0.0002",
                "--percent_dense", "0.001", "--svd_depth_warmup", "1", "--use_dust3r", "0", "--start_sample_svd_frame", "2000"]
# bash_scripts/batch_dl3dv_train.sh:84-87
DL3DV_LINE = ["--iteration", "dgs1", "--weight_clamp", "0.2", "--diffusion_type", "2PassProbUncertainPost", "--interp_type",
              "backward_warp", "--cam_confidence", "0.2", "--pseudo_cam_sampling_rate", "0.02", "--densify_type", "interpolate_gs_v2",
              "--dataset", "dl3dv", "--lpips_weight", "1", "--svd_l1_weight", "0", "--refine_cycle_num", "2", "--fps_keyframe_sampling",
              "1", "-s", "data/dl3dv/x", "--model_path", "out/x", "--eval", "--n_views", "6", "--sample_svd_pseudo_interval", "1",
              "--num_train_samples", "6", "--images", "images_4", "--resolution", "1", "--use_proximity_densify", "0",
              "--densify_grad_threshold", "0.0002", "--percent_dense", "0.001", "--svd_depth_warmup", "1", "--use_dust3r", "0",
              "--rand_pcd", "--start_sample_svd_frame", "2000"]


def test_llff_optimiser_flags_are_parsed_not_ignored():
    from syn3r_amd import launch
    args = launch.parse(["--scenes", "fern"] + LLFF_GS_ARGS)
    assert args.percent_dense == 0.001 and args.densify_grad_threshold == 0.0002
    assert "--percent_dense" not in args.ignored_flags and "--densify_grad_threshold" not in args.ignored_flags
    for flag in ("-s", "--eval", "--n_views", "--use_dust3r", "--sample_pseudo_interval", "--sample_svd_pseudo_interval", "--num_train_samples",
                 "--resolution", "--svd_depth_warmup", "--start_sample_svd_frame"):
        assert flag in args.ignored_flags, flag
    assert args.gs_schedule == "constant" and args.sh_degree is None and args.position_lr_final is None


def test_dl3dv_line_parses_and_a_misspelling_still_errors(capsys):
    from syn3r_amd import launch
    args = launch.parse(["--scenes", "x"] + DL3DV_LINE)
    assert args.percent_dense == 0.001 and args.lpips_weight == 1 and args.refine_cycle_num == 2
    assert "--svd_l1_weight" in args.ignored_flags and "--rand_pcd" in args.ignored_flags
    with pytest.raises(SystemExit):
        launch.parse(["--scenes", "x", "--percent_dens", "0.001"])
    assert "--percent_dens" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        launch.parse(["--scenes", "x", "--gs_schedule", "publishd"])


def test_apply_trainer_flags():
    from syn3r_amd import launch
    from syn3r_amd.gs.trainer import OptimizationParams
    base = OptimizationParams(iterations=77, lambda_dssim=0.3, seed=4)
    default = launch.parse(["--scenes", "x"])
    for flag, _ in launch.TRAINER_FLAGS:
        assert getattr(default, flag) is None
    out = launch.apply_trainer_flags(base, default)
    assert out == base and out == OptimizationParams(iterations=77, lambda_dssim=0.3, seed=4)
    # the new fields are off by default
    assert (base.position_lr_final, base.spatial_lr_scale, base.feature_rest_lr_div, base.sh_degree_interval) == (None, 1.0, 1.0, 0)
    values = {"percent_dense": 0.001, "densify_grad_threshold": 0.0003, "densify_from_iter": 11, "densify_until_iter": 1234,
              "densification_interval": 13, "opacity_reset_interval": 170, "position_lr_init": 3e-4, "position_lr_final": 3e-6,
              "position_lr_max_steps": 999, "feature_lr": 2e-3, "opacity_lr": 4e-2, "scaling_lr": 6e-3, "rotation_lr": 2e-3}
    argv = ["--scenes", "x", "--sh_degree", "2"]
    for k, v in values.items():
        argv += ["--" + k, repr(v)]
    args = launch.parse(argv)
    assert args.ignored_flags == [] and args.sh_degree == 2
    out = launch.apply_trainer_flags(base, args)
    expect = dict(values)
    expect["position_lr"] = expect.pop("position_lr_init")
    for k, v in expect.items():
        assert getattr(out, k) == v and type(getattr(out, k)) is type(v), k
    untouched = {f.name for f in dataclasses.fields(base)} - set(expect)
    assert all(getattr(out, k) == getattr(base, k) for k in untouched)
    assert base == OptimizationParams(iterations=77, lambda_dssim=0.3, seed=4)           # the argument is not modified
    # --gs_schedule published: the four switches; an explicit --position_lr_final wins over 1.6e-6
    pub = launch.apply_trainer_flags(base, launch.parse(["--scenes", "x", "--gs_schedule", "published"]))
    assert pub.position_lr_final == 1.6e-6 and pub.spatial_lr_scale is None and pub.feature_rest_lr_div == 20 and pub.sh_degree_interval == 1000
    assert pub.position_lr == base.position_lr and pub.position_lr_max_steps == 30_000 and pub.percent_dense == base.percent_dense
    pub = launch.apply_trainer_flags(base, launch.parse(["--scenes", "x", "--gs_schedule", "published", "--position_lr_final", "1e-5"]))
    assert pub.position_lr_final == 1e-5


def test_model_starts_at_a_lower_active_degree():
    """`GaussianModel(active_sh_degree=)` and `oneupSHdegree` need no device."""
    import torch
    from syn3r_amd.gs.trainer import GaussianModel
    mk = lambda **kw: GaussianModel(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 4), torch.zeros(2), torch.zeros(2, 16, 3),
                                    device="cpu", **kw)
    assert mk().active_sh_degree == 3 and mk(sh_degree=2).active_sh_degree == 2
    g = mk(active_sh_degree=0)
    assert (g.active_sh_degree, g.max_sh_degree) == (0, 3)
    seen = []
    for _ in range(5):
        g.oneupSHdegree()
        seen.append(g.active_sh_degree)
    assert seen == [1, 2, 3, 3, 3]
    with pytest.raises(ValueError):
        mk(active_sh_degree=4)
