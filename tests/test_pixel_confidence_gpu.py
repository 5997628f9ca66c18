"""`args.pixel_confidence = 1` through one refine cycle of the orchestrator (mock SVD components): the fused uncertainty of every
interpolated view pair reaches the finetune as per-pixel confidence maps on the pseudo-cameras and is cached beside the frames
(an extension: the reference weights a pseudo-view by the scalar `cam_confidence` alone)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import pipeline_mocks as PM
from oracle import raster_oracle as RO

pytestmark = pytest.mark.gpu

H, W = 72, 128


def build(gpu, tmp_path, iterations=5, N=800):
    """tests/test_diffusiongs_gpu.py's harness: three views of a synthetic scene, a perturbed model to train"""
    from syn3r_amd.gs import Camera, GaussianModel, GSTrainer, OptimizationParams
    m, s, q, o, sh = RO.synthetic_gaussians(N, seed=5, log_scale_mean=np.log(0.08))
    logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
    gt = GaussianModel(m, torch.log(s), q, logit, sh, device=gpu)
    f = W / (2 * math.tan(math.radians(30)))
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=np.float32)
    poses = []
    for dx in (-0.15, 0.0, 0.15):
        p = np.eye(4, dtype=np.float32)
        p[0, 3] = dx
        poses.append(p)
    tr_gt = GSTrainer(gt, [Camera.from_w2c(poses[0], K, H, W, data_device=gpu)])
    views = [tr_gt.render_view(Camera.from_w2c(p, K, H, W, data_device=gpu))["render"].detach() for p in poses]
    cams = [Camera.from_w2c(p, K, H, W, image=v, data_device=gpu) for p, v in zip(poses, views)]
    gm = GaussianModel(m + 0.01 * torch.randn_like(m), torch.log(s), q, logit, sh, device=gpu)
    trainer = GSTrainer(gm, cams, OptimizationParams(iterations=iterations), model_path=str(tmp_path / "model"),
                        checkpoint_iterations=[iterations])
    args = SimpleNamespace(cam_confidence=0.05, pseudo_cam_sampling_rate=0.5, fps_keyframe_sampling=0,
                           densify_type="interpolate_gs_v2", num_views_for_pcd_densification=1)
    return trainer, args


def _runner(gpu, tmp_path, **kw):
    from syn3r_amd.diffusionGS import DiffusionGS
    trainer, args = build(gpu, tmp_path)
    args.pixel_confidence = 1
    comps = dict(vae=PM.MockVAE(), image_encoder=PM.MockImageEncoder(), unet=PM.MockUNet().to(gpu), dtype=torch.float32)
    d = DiffusionGS(trainer, num_input_views=3, save_dir=str(tmp_path), diffusion_type="2PassProbUncertain", input_args=args,
                    svd_components=comps, num_inference_steps=2, **kw)
    return trainer, d


def test_one_refine_cycle_hands_the_uncertainty_to_the_finetune(gpu, tmp_path, monkeypatch):
    from syn3r_amd import orchestrator as O
    trainer, d = _runner(gpu, tmp_path, interp_type="backward_warp")
    uncs = []
    fuse = O.fuse_uncertainty_device

    def spy_fuse(*a, **k):
        out = fuse(*a, **k)
        uncs.append(out[2].detach().clone())
        return out

    monkeypatch.setattr(O, "fuse_uncertainty_device", spy_fuse)
    seen = {}
    finetune = trainer.finetune

    def spy_finetune(*a, **k):
        seen["maps"] = [c.confidence_map for c in trainer.pseudo_cameras]
        seen["conf"] = [c.cam_confidence for c in trainer.pseudo_cameras]
        return finetune(*a, **k)

    trainer.finetune = spy_finetune
    np.random.seed(0)
    d.run(refine_cycles=1)
    assert len(seen["maps"]) == 72 and set(seen["conf"]) == {0.05} and len(uncs) == 3
    for i in range(3):
        assert uncs[i].shape == (23, 576, 1024)
        assert seen["maps"][24 * i] is None                              # a pair's first frame is a real input view
        small = torch.nn.functional.interpolate(uncs[i][None], size=(H, W), mode="bilinear", align_corners=False)[0]
        for k in range(1, 24):
            m = seen["maps"][24 * i + k]
            assert m.shape == (H, W) and m.dtype == torch.float32 and m.is_cuda
            assert float(m.min()) >= 0.0 and float(m.max()) <= 1.0           # (NaN fails both)
            # 1 - resize(unc); where the fused uncertainty is undefined (NaN: no rendered depth under the pixel) the confidence is 0
            want = (1.0 - small[k - 1]).clamp(0, 1)
            assert bool((m[want.isnan()] == 0).all())
            torch.testing.assert_close(m, torch.nan_to_num(want, nan=0.0), rtol=0, atol=1e-6)
    assert any(float(m.min()) < float(m.max()) for m in seen["maps"] if m is not None)      # not a constant in disguise
    assert len(trainer.pseudo_cameras) == 0 and d.refine_epoch == 1
    # the caches carry the maps, and a second densify_views reloads the same ones
    files = sorted(p.name for p in tmp_path.iterdir() if p.suffix == ".pt")
    assert files == [f"dense_viewsinterpolated_dense_views_cyc0_view{i}.pt" for i in range(3)]
    data = torch.load(tmp_path / files[1], weights_only=False)
    assert sorted(data) == ["confidence_maps", "poses", "views"] and len(data["confidence_maps"]) == 25
    assert data["confidence_maps"][0] is None and data["confidence_maps"][-1] is None
    assert torch.equal(data["confidence_maps"][7], seen["maps"][24 + 7].cpu())
    n_fused = len(uncs)
    views, _, _ = d.densify_views(0, densify_type="interpolate_gs_v2", num_views_for_pcd_densification=1)
    assert len(uncs) == n_fused and len(views) == 72 and len(d.dense_confidence_maps) == 72
    for a, b in zip(d.dense_confidence_maps, seen["maps"]):
        assert (a is None and b is None) or torch.equal(a, b.cpu())
    # a cache written without the key loads as all None
    torch.save({"views": data["views"], "poses": data["poses"]}, tmp_path / files[1])
    d.densify_views(0, densify_type="interpolate_gs_v2", num_views_for_pcd_densification=1)
    assert all(m is None for m in d.dense_confidence_maps[24:48]) and d.dense_confidence_maps[1] is not None


def test_forward_warp_has_no_maps(gpu, tmp_path):
    trainer, d = _runner(gpu, tmp_path)
    assert d.interp_type == "forward_warp"
    np.random.seed(2)
    frames, poses, _ = d._interpolate_between_gs_v3(0, 1, replace=True, perturb_interp_poses=False)
    assert len(frames) == 25 and d._pair_confidence_maps == [None] * 25
