"""float64 reference of the anti-aliased rasteriser (the published `antialiasing` switch: Mip-Splatting's 2D Mip filter), built
from oracle/raster_oracle.py WITHOUT touching it and never from the code under test:

    1. RO.preprocess once; the dilated 2D covariance comes back out of its conic: d1 = 1 / (con0 con2 - con1^2), A = con2 d1,
       b = -con1 d1, C = con0 d1
    2. rho = sqrt(clamp(((A - 0.3)(C - 0.3) - b^2) / d1, min = 0.000025))
    3. RO.rasterize with opacities * rho: autograd carries the rho term into means, scales and rotations.

Shared by tests/test_raster_aa_cpu.py and tests/test_raster_aa_gpu.py; a reference is computed once per scene and cached."""
import math

import numpy as np
import torch

from oracle import raster_oracle as RO

LOW_PASS = 0.3
R_FLOOR = 0.000025
# (N, H, W, conf, deg, scale); the seed is N + H
SHAPES = [(400, 40, 72, False, 3, 0.06), (300, 33, 50, True, 1, 0.02), (800, 64, 64, True, 2, 0.01)]
PARAMS = ("m", "s", "q", "o", "sh")


def scene(N, H, W, conf, scale):
    """tests/test_raster_gpu.py::scene (5 Gaussians behind the camera, 5 far off-axis) plus 8 point-like Gaussians (they sit on the
    floor of rho) and 8 needles (the determinant cancels in fp32)."""
    seed = N + H
    m, s, q, o, sh = RO.synthetic_gaussians(N, seed=seed, dtype=torch.float64, log_scale_mean=np.log(scale))
    m[:5, 2] = -1.0
    m[5:10, 0] = 40.0
    s[10:18] = 1e-5
    s[18:26, 0] = 1e-6
    view, proj, campos, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float64)
    cf = None
    if conf:
        g = torch.Generator().manual_seed(seed + 1)
        cf = 0.2 + 0.8 * torch.rand(N, generator=g, dtype=torch.float64)
    bg = torch.tensor([0.1, 0.3, 0.7], dtype=torch.float64)
    return dict(m=m, s=s, q=q, o=o, sh=sh, cf=cf, view=view, proj=proj, campos=campos, tfx=tfx, tfy=tfy, bg=bg, H=H, W=W, N=N)


def rho_from_conic(conic):
    con0, con1, con2 = conic[:, 0], conic[:, 1], conic[:, 2]
    d1 = 1.0 / (con0 * con2 - con1 * con1)
    A, b, C = con2 * d1, -con1 * d1, con0 * d1
    r = ((A - LOW_PASS) * (C - LOW_PASS) - b * b) / d1
    return torch.sqrt(torch.clamp(r, min=R_FLOOR)), r


def rasterize(sc, deg, antialiasing=True, requires_grad=False, conf_grad=False):
    """-> ((color, radii, depth, alpha, aux), params dict, rho, r) in float64; `params["cf"]` requires grad with `conf_grad`."""
    f = lambda t: t.to(torch.float64).clone().requires_grad_(requires_grad)
    p = {k: f(sc[k]) for k in PARAMS}
    p["cf"] = None
    if sc["cf"] is not None:
        p["cf"] = sc["cf"].to(torch.float64).clone().requires_grad_(requires_grad and conf_grad)
    cam = (sc["view"], sc["proj"], sc["campos"], sc["tfx"], sc["tfy"], sc["H"], sc["W"])
    rho = r = None
    op = p["o"]
    if antialiasing:
        pre = RO.preprocess(p["m"], p["s"], p["q"], p["o"], p["sh"], p["cf"], *cam, deg)
        rho, r = rho_from_conic(pre["conic"])
        op = p["o"] * rho
    out = RO.rasterize(p["m"], p["s"], p["q"], op, p["sh"], p["cf"], *cam, sc["bg"], deg)
    return out, p, rho, r


_cache = {}


def loss_weights(H, W):
    """the weights of tests/test_raster_gpu.py::test_backward_vs_autograd"""
    g = torch.Generator().manual_seed(3)
    wc = torch.randn(3, H, W, generator=g, dtype=torch.float64)
    wd = 0.3 * torch.randn(1, H, W, generator=g, dtype=torch.float64)
    wa = torch.randn(1, H, W, generator=g, dtype=torch.float64)
    return wc, wd, wa


def reference(shape):
    """The scene of one of SHAPES with its float64 renders (filter on and off) and the gradients of
    sum(wc colour) + sum(wd depth) + sum(wa alpha) with the filter on.  Computed once; callers must not modify it."""
    if shape not in _cache:
        N, H, W, conf, deg, scale = shape
        sc = scene(N, H, W, conf, scale)
        (oc, orad, od, oa, aux), p, rho, r = rasterize(sc, deg, True, requires_grad=True, conf_grad=True)
        wc, wd, wa = loss_weights(H, W)
        ((oc * wc).sum() + (od * wd).sum() + (oa * wa).sum()).backward()
        grads = {k: p[k].grad.clone() for k in PARAMS}
        if conf:
            grads["cf"] = p["cf"].grad.clone()
        with torch.no_grad():
            (fc, frad, fd, fa, _), _, _, _ = rasterize(sc, deg, False)
        valid = aux["pre"]["valid"]
        _cache[shape] = dict(sc=sc, deg=deg, color=oc.detach(), depth=od.detach(), alpha=oa.detach(), radii=orad, grads=grads,
                             rho=rho.detach(), r=r.detach(), valid=valid, color_off=fc, alpha_off=fa, weights=(wc, wd, wa))
    return _cache[shape]


def single_gaussian(z, H=64, W=64):
    """One isotropic Gaussian, scale 0.02, opacity 0.8, SH degree 0, at (0.013 z, -0.021 z, z); black background, 60 degree fov."""
    m = torch.tensor([[0.013 * z, -0.021 * z, z]], dtype=torch.float64)
    s = torch.full((1, 3), 0.02, dtype=torch.float64)
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    o = torch.tensor([0.8], dtype=torch.float64)
    sh = torch.zeros(1, 16, 3, dtype=torch.float64)
    sh[:, 0] = 1.0
    view, proj, campos, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float64)
    bg = torch.zeros(3, dtype=torch.float64)
    return dict(m=m, s=s, q=q, o=o, sh=sh, cf=None, view=view, proj=proj, campos=campos, tfx=tfx, tfy=tfy, bg=bg, H=H, W=W, N=1)


def footprint(sc, z):
    """op 2 pi sigma_px^2: the alpha an isotropic Gaussian of scale 0.02 at depth z deposits without any dilation"""
    fx = sc["W"] / (2.0 * sc["tfx"])
    return float(sc["o"][0]) * 2.0 * math.pi * (fx * 0.02 / z) ** 2
