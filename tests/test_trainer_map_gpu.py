"""`Camera.confidence_map` in the trainer: the per-pixel weight reaches the photometric loss on the explicit step and on the
autograd step alike (an extension: the reference's camera carries the scalar `cam_confidence` only)."""
import math

import numpy as np
import pytest
import torch

from oracle import raster_oracle as RO

pytestmark = pytest.mark.gpu

N, H, W = 3000, 72, 104


def make_scene(N, H, W, seed, dev):
    """tests/test_trainer_gpu.py's scene"""
    from syn3r_amd.gs import GaussianModel
    m, s, q, o, sh = RO.synthetic_gaussians(N, seed=seed, log_scale_mean=np.log(0.08))
    logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
    gm = GaussianModel(m, torch.log(s), q, logit, sh, device=dev)
    K = np.array([[W / (2 * math.tan(math.radians(30))), 0, W / 2], [0, W / (2 * math.tan(math.radians(30))), H / 2],
                  [0, 0, 1]], dtype=np.float32)
    return gm, K


def _target():
    return torch.rand(3, H, W, generator=torch.Generator().manual_seed(5))


def _step(gpu, lambda_dssim, explicit, cam_confidence, cmap):
    """[loss, raw-parameter gradients ..., screen-space gradient] of one step on a fresh copy of the scene"""
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    gm, K = make_scene(N, H, W, 7, gpu)
    cam = Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, image=_target(), data_device=gpu, cam_confidence=cam_confidence,
                          confidence_map=cmap)
    tr = GSTrainer(gm, [cam], OptimizationParams(iterations=1, lambda_dssim=lambda_dssim))
    if explicit:
        loss, out = tr._explicit_step(cam)
        vs = out["viewspace_grad"]
    else:
        from syn3r_amd.gs.train_ops import l1_loss, photometric_loss
        out = tr.render_view(cam)
        loss = (photometric_loss(out["render"], cam.original_image, lambda_dssim, cam_confidence, weight_map=cam.confidence_map)
                if lambda_dssim > 0 else l1_loss(out["render"], cam.original_image, weight=cam_confidence, weight_map=cam.confidence_map))
        loss.backward()
        vs = out["viewspace_points"].grad
    return [float(loss)] + [p.grad.detach().clone() for p in gm.parameters()] + [vs.detach().clone()]


def _assert_same(a, b, measurements, name, **tags):
    worst = 0.0
    assert abs(a[0] - b[0]) < 1e-6
    for x, y in zip(a[1:], b[1:]):
        assert x.shape == y.shape
        scale = float(y.abs().max()) + 1e-20
        worst = max(worst, float((x - y).abs().max()) / scale)
        assert float((x - y).abs().max()) <= 2e-5 * scale, (float((x - y).abs().max()), scale)
    measurements(name, loss_err=abs(a[0] - b[0]), worst_rel_grad_err=worst, **tags)


@pytest.mark.parametrize("lambda_dssim", [0.2, 0.0])
def test_explicit_step_equals_autograd_step_with_a_map(lambda_dssim, gpu, measurements):
    cmap = torch.rand(H, W, generator=torch.Generator().manual_seed(6))
    ex = _step(gpu, lambda_dssim, True, 0.7, cmap)
    au = _step(gpu, lambda_dssim, False, 0.7, cmap)
    _assert_same(ex, au, measurements, "trainer_map_explicit_vs_autograd", lam=lambda_dssim)
    # the map is in the loss: the same step without it is another loss
    assert abs(ex[0] - _step(gpu, lambda_dssim, True, 0.7, None)[0]) > 1e-3
    # and train_step's own two branches read it too: the same first Adam update (lr * sign(grad))
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    finals = []
    for explicit in (None, False):
        gm, K = make_scene(N, H, W, 7, gpu)
        cam = Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, image=_target(), data_device=gpu, cam_confidence=0.7)
        cam.confidence_map = cmap                                     # settable as an attribute
        tr = GSTrainer(gm, [cam], OptimizationParams(iterations=1, lambda_dssim=lambda_dssim))
        loss = tr.train_step(cam, explicit=explicit)
        assert abs(float(loss) - ex[0]) < 1e-6
        finals.append([p.detach().clone() for p in gm.parameters()])
    for a, b in zip(*finals):
        assert ((a - b).abs() > 1e-6).double().mean() < 1e-3


@pytest.mark.parametrize("lambda_dssim", [0.2, 0.0])
def test_map_of_zeros_gives_zero_gradients(lambda_dssim, gpu):
    r = _step(gpu, lambda_dssim, True, 0.7, torch.zeros(H, W))
    assert r[0] == 0.0
    for g in r[1:]:
        assert bool((g == 0).all())


@pytest.mark.parametrize("lambda_dssim", [0.2, 0.0])
def test_constant_map_is_a_scalar_confidence(lambda_dssim, gpu, measurements):
    a = _step(gpu, lambda_dssim, True, 0.7, torch.full((H, W), 0.5))
    b = _step(gpu, lambda_dssim, True, 0.35, None)
    _assert_same(a, b, measurements, "trainer_map_constant", lam=lambda_dssim)


def test_update_cameras_registers_maps(gpu):
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    gm, K = make_scene(200, 24, 32, 3, gpu)
    cam = Camera.from_w2c(np.eye(4, dtype=np.float32), K, 24, 32, image=torch.rand(3, 24, 32), data_device=gpu)
    tr = GSTrainer(gm, [cam], OptimizationParams(iterations=1))
    views = [torch.rand(3, 24, 32) for _ in range(3)]
    poses = [np.eye(4, dtype=np.float32)] * 3
    maps = [None, torch.rand(24, 32), torch.rand(1, 24, 32).double()]
    tr.update_cameras(views, poses, K, 0.1, confidence_maps=maps)
    ps = tr.pseudo_cameras
    assert len(ps) == 3 and ps[0].confidence_map is None
    for c, m in zip(ps[1:], maps[1:]):
        assert c.confidence_map.shape == (24, 32) and c.confidence_map.dtype == torch.float32 and c.confidence_map.device.type == "cuda"
        assert torch.equal(c.confidence_map.cpu(), m.reshape(24, 32).float()) and c.cam_confidence == 0.1
    tr.train_step(ps[1])                                              # a registered map trains
    tr.update_cameras(views, poses, K, 0.1, append=False)              # without maps: as before
    assert all(c.confidence_map is None for c in tr.pseudo_cameras)
    with pytest.raises(ValueError):
        tr.update_cameras(views, poses, K, 0.1, confidence_maps=maps[:2])
    with pytest.raises(ValueError):
        tr.update_cameras(views, poses, K, 0.1, confidence_maps=[None, None, torch.rand(32, 24)])
