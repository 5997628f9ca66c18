"""float64 reference of the ABSOLUTE screen-space gradient (AbsGS, Ye et al. 2024, section 3.2; syn3r_raster_backward_abs), built from
oracle/raster_oracle.py WITHOUT touching it and never from the code under test:

    1. `blend_tile` restates RO.blend_tile with two extra leaf tensors ex, ey of shape [n_splats, n_pixels], all zeros, in the
       offsets: dx = px[:, None] + ex - pxf[None], dy likewise.  Same arithmetic otherwise (tests/test_raster_absgrad_cpu.py pins its
       outputs to RO.render's exactly).
    2. one autograd.grad of the tile's loss sum(wc colour) + sum(wd depth) + sum(wa alpha) with respect to (ex, ey) is EVERY
       per-(splat, pixel) gradient of the loss with respect to the projected mean, in pixels.
    3. the reference is 0.5 W sum_p |dL/dex| and 0.5 H sum_p |dL/dey| (the units of dL_dmeans2D: NDC), index-added over the tiles;
       the plain sums sum_p dL/dex, sum_p dL/dey (pixels) come along - they are RO.render_with_grads' px / py gradients.

It takes the blend inputs `pre`, the point list, the ranges and the weights, so it serves every mode: the plain render
(RO.rasterize's aux), the anti-aliased one (raster_aa_ref.rasterize's aux) and the filtered one (raster_f3d_ref.rasterize's).
Scenes: raster_aa_ref.SHAPES, a fourth opaque one (the blend's early stop) and a single symmetric Gaussian (exact cancellation of the
plain sum).  A reference is computed once per key and cached; callers must not modify it."""
import numpy as np
import torch

import raster_aa_ref as A
from oracle import raster_oracle as RO

OPAQUE = (800, 64, 64, False, 2, 0.15)            # (N, H, W, conf, deg, scale) of the fourth scene: every opacity 0.99
SCENES = list(A.SHAPES) + [OPAQUE]
SCENE_IDS = [f"N{s[0]}_{s[1]}x{s[2]}" for s in A.SHAPES] + ["opaque_N800_64x64"]


def blend_tile(px, py, conic, rgb, zdepth, opacity, pxf, pyf, bg, ex, ey):
    """RO.blend_tile with the per-(splat, pixel) offsets (ex, ey) added to the mean: -> colour [npix,3], depth, alpha, n_contrib."""
    dt = px.dtype
    dx = px[:, None] + ex - pxf[None]
    dy = py[:, None] + ey - pyf[None]
    power = -0.5 * (conic[:, 0:1] * dx * dx + conic[:, 2:3] * dy * dy) - conic[:, 1:2] * dx * dy
    raw = opacity[:, None] * torch.exp(power)
    alpha = raw - torch.clamp(raw - 0.99, min=0).detach()     # min(0.99, raw), straight-through
    ok = (power <= 0) & (alpha >= 1.0 / 255.0)
    a_eff = torch.where(ok, alpha, torch.zeros_like(alpha))
    one_m = 1.0 - a_eff
    T_incl = torch.cumprod(one_m, 0)
    T_excl = torch.cat([torch.ones(1, T_incl.shape[1], dtype=dt), T_incl[:-1]], 0)
    stop = ok & (T_incl < 1e-4)
    stopped = torch.cummax(stop.to(torch.int8), 0)[0].bool()
    live = ok & ~stopped
    w = torch.where(live, a_eff * T_excl, torch.zeros_like(a_eff))
    T_final = torch.prod(torch.where(live, one_m, torch.ones_like(one_m)), 0)
    c = (w[:, :, None] * rgb[:, None, :]).sum(0) + T_final[:, None] * bg.to(dt)[None]
    d = (w * zdepth[:, None]).sum(0)
    idx = torch.arange(1, live.shape[0] + 1)[:, None] * live
    return c, d, 1.0 - T_final, idx.max(0)[0]


def abs_reference(pre, point_list, ranges, bg, H, W, wc, wd, wa):
    """-> dict(abs [N,2] NDC units, signed_px [N,2] pixel units, color, depth, alpha, lists: the tile lists' lengths)."""
    dt = pre["px"].dtype
    gx, gy = pre["grid"]
    N = pre["px"].shape[0]
    color = torch.zeros(3, H, W, dtype=dt) + bg.to(dt)[:, None, None]
    depth = torch.zeros(1, H, W, dtype=dt)
    alpha = torch.zeros(1, H, W, dtype=dt)
    absg, signed = torch.zeros(N, 2, dtype=dt), torch.zeros(N, 2, dtype=dt)
    lists = []
    for ty in range(gy):
        for tx in range(gx):
            s, e = ranges[ty * gx + tx]
            hh, ww, pxf, pyf = RO._tile_pixels(ty, tx, H, W, dt)
            if e <= s or hh == 0 or ww == 0:
                continue
            lists.append(int(e - s))
            ids = torch.from_numpy(point_list[s:e])
            loc = [pre[k][ids].detach() for k in RO.BLEND_KEYS]
            ex = torch.zeros(len(ids), hh * ww, dtype=dt, requires_grad=True)
            ey = torch.zeros(len(ids), hh * ww, dtype=dt, requires_grad=True)
            c, d, a, _ = blend_tile(*loc, pxf, pyf, bg, ex, ey)
            y0, x0 = ty * RO.TILE, tx * RO.TILE
            sl = (slice(y0, y0 + hh), slice(x0, x0 + ww))
            loss = ((c.T.reshape(3, hh, ww) * wc[(slice(None),) + sl]).sum() + (d.reshape(hh, ww) * wd[(0,) + sl]).sum()
                    + (a.reshape(hh, ww) * wa[(0,) + sl]).sum())
            gex, gey = torch.autograd.grad(loss, [ex, ey])
            absg.index_add_(0, ids, torch.stack([0.5 * W * gex.abs().sum(1), 0.5 * H * gey.abs().sum(1)], 1))
            signed.index_add_(0, ids, torch.stack([gex.sum(1), gey.sum(1)], 1))
            color[(slice(None),) + sl] = c.detach().T.reshape(3, hh, ww)
            depth[(0,) + sl] = d.detach().reshape(hh, ww)
            alpha[(0,) + sl] = a.detach().reshape(hh, ww)
    return dict(abs=absg, signed_px=signed, color=color, depth=depth, alpha=alpha, lists=lists)


def from_aux(sc, aux, weights):
    """The reference of a float64 render `aux` (RO.rasterize's fifth output, or that of the two mode references) of scene `sc`."""
    return abs_reference(aux["pre"], aux["point_list"], aux["ranges"], sc["bg"], sc["H"], sc["W"], *weights)


def weights_of(H, W, depth_grad=True):
    """raster_aa_ref.loss_weights; without a depth gradient wd is zero (the caller hands the kernel no dL_ddepth)"""
    wc, wd, wa = A.loss_weights(H, W)
    return wc, (wd if depth_grad else torch.zeros_like(wd)), wa


def make_scene(shape):
    N, H, W, conf, deg, scale = shape
    sc = A.scene(N, H, W, conf, scale)
    if shape == OPAQUE:
        sc["o"] = torch.full_like(sc["o"], 0.99)
    return sc


def plain_aux(sc, deg):
    with torch.no_grad():
        out = RO.rasterize(sc["m"], sc["s"], sc["q"], sc["o"], sc["sh"], sc["cf"], sc["view"], sc["proj"], sc["campos"], sc["tfx"],
                           sc["tfy"], sc["H"], sc["W"], sc["bg"], deg)
    return out


_cache = {}


def reference(shape, depth_grad=True):
    """Plain-mode reference of one of SCENES: dict(sc, deg, aux, weights, valid, and abs_reference's keys).  Computed once."""
    key = (shape, bool(depth_grad))
    if key not in _cache:
        sc, deg = make_scene(shape), shape[4]
        color, radii, depth, alpha, aux = plain_aux(sc, deg)
        weights = weights_of(sc["H"], sc["W"], depth_grad)
        ref = from_aux(sc, aux, weights)
        ref.update(sc=sc, deg=deg, aux=aux, weights=weights, valid=aux["pre"]["valid"], oracle=(color, depth, alpha))
        _cache[key] = ref
    return _cache[key]


def cancel_scene(H=64, W=64):
    """One isotropic Gaussian at (0, 0, 2): scale 0.3, opacity 0.5, SH degree 0.  It projects to (31.5, 31.5), between four pixels:
    the image is symmetric about it in x and in y, and with a constant colour weight the per-pixel gradients cancel exactly."""
    m = torch.tensor([[0.0, 0.0, 2.0]], dtype=torch.float64)
    s = torch.full((1, 3), 0.3, dtype=torch.float64)
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    o = torch.tensor([0.5], dtype=torch.float64)
    sh = torch.zeros(1, 16, 3, dtype=torch.float64)
    sh[:, 0] = 1.0
    view, proj, campos, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float64)
    bg = torch.zeros(3, dtype=torch.float64)
    return dict(m=m, s=s, q=q, o=o, sh=sh, cf=None, view=view, proj=proj, campos=campos, tfx=tfx, tfy=tfy, bg=bg, H=H, W=W, N=1)


def cancel_weights(H=64, W=64):
    return (torch.ones(3, H, W, dtype=torch.float64), torch.zeros(1, H, W, dtype=torch.float64),
            torch.zeros(1, H, W, dtype=torch.float64))


def cancel_reference():
    if "cancel" not in _cache:
        sc = cancel_scene()
        _, _, _, _, aux = plain_aux(sc, 0)
        weights = cancel_weights()
        ref = from_aux(sc, aux, weights)
        ref.update(sc=sc, deg=0, aux=aux, weights=weights)
        _cache["cancel"] = ref
    return _cache["cancel"]


def norms(ref):
    """(abs norm [N], plain norm [N]) in NDC units"""
    sc = ref["sc"]
    plain = ref["signed_px"] * torch.tensor([0.5 * sc["W"], 0.5 * sc["H"]], dtype=torch.float64)
    return ref["abs"].norm(dim=1), plain.norm(dim=1)
