"""TEST INFRASTRUCTURE - what tests/test_lpips_split_cpu.py and tests/test_lpips_split_gpu.py share: the seeded weights and images
of tests/test_lpips_gpu.py::test_lpips_value_and_gradient_vs_oracle, and a float64 restatement of oracle/lpips_oracle.py into which
the individual roundings of the HIP path can be inserted (`emulate`); tests/test_lpips_gpu.py takes its images, weights and trainer
setup from here too."""
import math

import torch
import torch.nn.functional as Fn

from oracle import lpips_oracle as LO

LOSS_SCALE_PER_PIXEL = 1024.0      # syn3r_amd.gs.lpips.LPIPS.LOSS_SCALE_PER_PIXEL


def images(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(xs / 7 + c) * torch.cos(ys / 5 - c) for c in range(3)])
    a = (base + 0.08 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    b = (base.roll(2, 2) + 0.08 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    return a, b


def seeded_state_dict(shapes, seed=3):
    """The draws of LPIPS.init_random(seed)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in shapes.items():
        if k.startswith("lin"):
            sd[k] = torch.rand(shape, generator=g) * 0.2 + 0.01
        elif k.endswith(".bias"):
            sd[k] = 0.05 * torch.randn(shape, generator=g)
        else:
            sd[k] = torch.randn(shape, generator=g) * math.sqrt(2.0 / (shape[1] * 9))
    return sd


def parameter_shapes():
    from syn3r_amd.gs.lpips import LPIPS
    return LPIPS().parameter_shapes()


def trainer_with_lpips(gpu, precision):
    """The trainer-step tests' setup: 600 Gaussians seen by one 48 x 64 camera whose image is their own render, a GSTrainer on a
    perturbed copy (lpips_weight 1, the term still switched off) with a seeded LPIPS of `precision` attached -> (trainer, camera)."""
    import numpy as np
    from oracle import raster_oracle as RO
    from syn3r_amd.gs import Camera, GaussianModel, GSTrainer, OptimizationParams
    from syn3r_amd.gs.lpips import LPIPS
    N, H, W = 600, 48, 64
    mm, s, q, o, sh = RO.synthetic_gaussians(N, seed=2, log_scale_mean=np.log(0.08))
    logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
    f = W / (2 * math.tan(math.radians(30)))
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=np.float32)
    gt = GSTrainer(GaussianModel(mm, torch.log(s), q, logit, sh, device=gpu), [Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, data_device=gpu)])
    img = gt.render_view(gt.scene.getTrainCameras()[0])["render"].detach().clamp(0, 1)
    cam = Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, image=img, data_device=gpu)
    gm = GaussianModel(mm + 0.02 * torch.randn_like(mm), torch.log(s), q, logit, sh, device=gpu)
    tr = GSTrainer(gm, [cam], OptimizationParams(iterations=3, lpips_weight=1.0))
    tr.lpips = LPIPS(precision=precision).init_random(gpu, seed=1)
    return tr, cam


def round_fp16(x):
    return x.half().to(x.dtype)


def round_fp16x2(x):
    """v (as fp32, the accumulator's format) -> float(half(v)) + float(half(v - float(half(v))))."""
    v = x.float()
    hi = v.half()
    lo = (v - hi.float()).half()
    return (hi.float() + lo.float()).to(x.dtype)


class _StoreAs(torch.autograd.Function):
    """Forward: the activation as it is stored (`act`); backward: the gradient as it is stored - fp16 of (gradient x scale),
    saturated, when `scale` > 0.  The rounding itself has no derivative on the HIP path (it is what the next kernel reads)."""

    @staticmethod
    def forward(ctx, x, act, scale):
        ctx.scale = scale
        return act(x) if act is not None else x.clone()

    @staticmethod
    def backward(ctx, g):
        if ctx.scale > 0:
            g = (g * ctx.scale).clamp(-65504.0, 65504.0).half().to(g.dtype) / ctx.scale
        return g, None, None


def emulate(pred, target, sd, act=None, target_act="same", grad_fp16=False):
    """oracle/lpips_oracle.py::lpips in the dtype of `pred` (float64 here) with fp16 weights, where every stored activation of the
    rendered image's branch goes through `act` (None: exact), of the target's branch through `target_act` ("same": `act`), and,
    with `grad_fp16`, every inter-layer gradient is stored as fp16 under the loss scale 1024 H W."""
    if target_act == "same":
        target_act = act
    q = lambda t: t.half().to(pred.dtype)
    scale = LOSS_SCALE_PER_PIXEL * pred.shape[1] * pred.shape[2] if grad_fp16 else 0.0

    def features(x, a, s_):
        x = ((2 * x[None] - 1) - LO.SHIFT.to(x.dtype)) / LO.SCALE.to(x.dtype)
        x = _StoreAs.apply(x, a, s_)
        out = []
        for s, idxs in enumerate(LO.SLICES):
            if s > 0:
                x = Fn.max_pool2d(x, 2, 2)
            for i in idxs:
                x = Fn.relu(Fn.conv2d(x, q(sd[f"net.slice{s + 1}.{i}.weight"]), q(sd[f"net.slice{s + 1}.{i}.bias"]), padding=1))
                x = _StoreAs.apply(x, a, s_)
            out.append(x)
        return out

    fa = features(pred, act, scale)
    with torch.no_grad():
        fb = features(target, target_act, 0.0)
    total = 0
    for k, (a, b) in enumerate(zip(fa, fb)):
        na = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        nb = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        total = total + ((na - nb) ** 2 * sd[f"lin{k}.model.1.weight"].to(pred.dtype)).sum(1).mean()
    return total


def grad_error(g, ref):
    """(relative error, cosine) of a gradient against the reference, both float64 CPU."""
    return float((g - ref).norm() / ref.norm()), float((g * ref).sum() / (g.norm() * ref.norm()))
