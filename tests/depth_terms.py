"""What the trainer tests of the three depth terms share (test_depth_loss_gpu, test_depth_local_gpu, test_depth_smooth_gpu): the
scene, a prior from another cloud, and the harness that reads the loss gradients the explicit step hands the rasteriser's backward."""
import numpy as np
import torch


def scene(N, H, W, seed, dev):
    from tests.test_trainer_gpu import make_scene
    return make_scene(N, H, W, seed, dev)


def prior(H, W, K, dev, seed=21):
    """A disparity prior from ANOTHER cloud: correlated with nothing in particular, so the term has work to do."""
    from syn3r_amd.gs import Camera, GSTrainer
    from syn3r_amd.launch import truth_disparity
    gm, _ = scene(2000, H, W, seed, dev)
    cam = Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, data_device=dev)
    return truth_disparity(GSTrainer(gm, [cam]), cam)


def spy_rasterize_backward(monkeypatch):
    """-> the list that receives (g_color, g_depth or None) of every `raster.rasterize_backward` call from now on"""
    from syn3r_amd import raster
    seen = []
    real_bwd = raster.rasterize_backward

    def spy(st, g_color, g_depth=None, g_alpha=None, **kw):
        seen.append((g_color.clone(), None if g_depth is None else g_depth.clone()))
        return real_bwd(st, g_color, g_depth, g_alpha, **kw)
    monkeypatch.setattr(raster, "rasterize_backward", spy)
    return seen


def step_bits(tr, cam, seen):
    """The explicit step's loss and the loss gradients it hands the rasteriser's backward (bitwise: both come from fixed-order
    kernels), and the parameter gradients (the rasteriser's backward accumulates with float atomics: equal to rounding)."""
    seen.clear()
    loss, out = tr._explicit_step(cam)
    (g_color, g_depth), = seen
    return [loss.clone(), g_color, g_depth], [p.grad.detach().clone() for p in tr.gaussians.parameters()] + [out["viewspace_grad"].clone()]


def same(a, b):
    bits_a, grads_a = a
    bits_b, grads_b = b
    assert torch.equal(bits_a[0], bits_b[0]) and torch.equal(bits_a[1], bits_b[1])
    assert (bits_a[2] is None) == (bits_b[2] is None) and (bits_a[2] is None or torch.equal(bits_a[2], bits_b[2]))
    for x, y in zip(grads_a, grads_b):
        assert float((x - y).abs().max()) <= 2e-5 * (float(y.abs().max()) + 1e-20)
