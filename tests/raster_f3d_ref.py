"""float64 reference of Mip-Splatting's 3D smoothing filter (syn3r_filter3d_compute, syn3r_raster_preprocess_f3d / _backward_f3d),
built from oracle/raster_oracle.py and tests/raster_aa_ref.py WITHOUT touching either and never from the code under test:

    1. the filter itself (`filter_reference`): per Gaussian and camera the view-space point, the visibility test, the minimum of
       z / fx over the seeing cameras, times sqrt(variance); unseen Gaussians take the largest seen filter, all zero if none is seen
    2. s' = sqrt(s^2 + f^2), o' = o prod(s / s'), then RO.rasterize(s', o'); with anti-aliasing o' rho, rho by raster_aa_ref's
       function from the conic of the FILTERED scales.  Autograd carries coef into the scales and rho into everything.

Scenes are raster_aa_ref.SHAPES (behind-camera, off-axis, point-like and needle Gaussians included); their filters come from
`filter_reference` over three look-at cameras at different distances.  Gaussians whose float64 radius argument 3 sqrt(lambda) lies
within 1e-4 of an integer are taken out of a scene (an fp32 radius may land on the other side; tests/test_filter3d_cpu.py holds the
count under 1 % of N).  A reference is computed once per (shape, anti-aliasing) and cached; callers must not modify it."""
import math

import numpy as np
import torch

import raster_aa_ref as A
from oracle import raster_oracle as RO

VARIANCE, NEAR, MARGIN = 0.2, 0.2, 0.15          # the recalled constants of the released code (UNPINNED), as the header has them
EPS32 = float(np.finfo(np.float32).eps)
RADIUS_EDGE = 1e-4
EYES = ((0.0, 0.0, 0.0), (0.3, 0.0, -2.0), (-0.2, 0.1, 1.0))      # the three look-at cameras of a scene's filter


def camera_row(view_t, tanfovx, tanfovy, H, W):
    """One row of the [C,16] camera table from an FSGS-style TRANSPOSED world-to-view matrix: [R | t] row by row, fx, fy, W, H."""
    w2c = view_t.to(torch.float64).t()
    fx, fy = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    return torch.cat([w2c[:3, :].reshape(-1), torch.tensor([fx, fy, float(W), float(H)], dtype=torch.float64)])


def scene_cameras(H, W):
    rows = []
    for e in EYES:
        view, _, _, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float64, eye=e)
        rows.append(camera_row(view, tfx, tfy, H, W))
    return torch.stack(rows)


def filter_reference(xyz, table, variance=VARIANCE, near=NEAR, margin=MARGIN):
    """-> dict(filter [N], seen [N] bool, margin_n [N] / margin_rel: the smallest relative distance of a Gaussian's (of any)
    (Gaussian, camera) pair to one of the visibility thresholds, front_any [N]: in front of some camera, bound [N]: the relative error an fp32 evaluation of a SEEN Gaussian's filter may have,
    16 eps32 (|row| . |p| + |t|) / z at the camera that gives the minimum (|row| . |p| = sum_i |row_i| |p_i|: the rounding-error bound of
    the fp32 dot product that forms z, with room for the division by fx, sqrt(variance) and the product)).  Everything in float64,
    from the values given (hand in the fp32-rounded inputs of the kernel to compare with it)."""
    p, T = xyz.to(torch.float64), table.to(torch.float64)
    Rm, t = T[:, :12].reshape(-1, 3, 4)[:, :, :3], T[:, :12].reshape(-1, 3, 4)[:, :, 3]
    fx, fy, W, H = T[:, 12], T[:, 13], T[:, 14], T[:, 15]
    v = torch.einsum("cij,nj->nci", Rm, p) + t[None]                    # [N, C, 3]
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    front = z > near
    zs = torch.where(front, z, torch.ones_like(z))
    u, w = fx * x / zs + 0.5 * W, fy * y / zs + 0.5 * H
    inside = (u >= -margin * W) & (u <= (1 + margin) * W) & (w >= -margin * H) & (w <= (1 + margin) * H)
    seen_nc = front & inside
    # relative distance to the thresholds: z against near for every pair, the pixel against the four edges for pairs in front
    rel = [((z - near).abs() / near).min(dim=1).values]
    for val, lo, hi, size in ((u, -margin * W, (1 + margin) * W, W), (w, -margin * H, (1 + margin) * H, H)):
        d = torch.minimum((val - lo).abs(), (val - hi).abs()) / size
        rel.append(torch.where(front, d, torch.full_like(d, math.inf)).min(dim=1).values)
    margin_n = torch.stack(rel).min(dim=0).values
    zf = torch.where(seen_nc, z / fx, torch.full_like(z, math.inf))
    best, arg = zf.min(dim=1)
    seen = seen_nc.any(dim=1)
    filt = math.sqrt(variance) * best
    mx = filt[seen].max() if bool(seen.any()) else torch.zeros((), dtype=torch.float64)
    filt = torch.where(seen, filt, mx)
    idx = torch.arange(p.shape[0])
    cond = (Rm[arg, 2].abs() * p.abs()).sum(1) + t[arg, 2].abs()
    bound = 16.0 * EPS32 * cond / z[idx, arg].abs().clamp_min(1e-300)
    return dict(filter=filt, seen=seen, margin_rel=float(margin_n.min()), margin_n=margin_n, bound=bound, front_any=front.any(dim=1))


def filtered(s, o, f):
    """(s', o') of the method: s' = sqrt(s^2 + f^2) per axis, o' = o prod(s / s')."""
    sf = torch.sqrt(s * s + (f * f)[:, None])
    return sf, o * (s / sf).prod(dim=1)


def lam_max(conic):
    """the larger eigenvalue of the dilated 2D covariance, back out of its conic (as raster_aa_ref.rho_from_conic does)"""
    con0, con1, con2 = conic[:, 0], conic[:, 1], conic[:, 2]
    d1 = 1.0 / (con0 * con2 - con1 * con1)
    a, c = con2 * d1, con0 * d1
    mid = 0.5 * (a + c)
    return mid + torch.sqrt(torch.clamp(mid * mid - d1, min=0.1))


_scene_cache = {}


def scene(shape):
    """raster_aa_ref.scene of `shape` with its per-Gaussian filters (key "f") and WITHOUT the Gaussians on a radius edge; "dropped"
    is their number, "N0" the size before.  Computed once."""
    if shape not in _scene_cache:
        N, H, W, conf, deg, scale = shape
        sc = A.scene(N, H, W, conf, scale)
        f = filter_reference(sc["m"], scene_cameras(H, W))["filter"]
        sf, of = filtered(sc["s"], sc["o"], f)
        pre = RO.preprocess(sc["m"], sf, sc["q"], of, sc["sh"], sc["cf"], sc["view"], sc["proj"], sc["campos"], sc["tfx"], sc["tfy"],
                            H, W, deg)
        arg = 3.0 * torch.sqrt(lam_max(pre["conic"]))
        edge = pre["valid"] & ((arg - torch.round(arg)).abs() < RADIUS_EDGE)
        keep = ~edge
        out = dict(sc)
        for k in A.PARAMS:
            out[k] = sc[k][keep].clone()
        out["cf"] = sc["cf"][keep].clone() if sc["cf"] is not None else None
        out["f"], out["N"], out["N0"], out["dropped"] = f[keep].clone(), int(keep.sum()), N, int(edge.sum())
        _scene_cache[shape] = out
    return _scene_cache[shape]


def rasterize(sc, deg, f, antialiasing, requires_grad=False):
    """-> ((color, radii, depth, alpha, aux), params dict) in float64; with `requires_grad` every parameter and the confidence
    require grad."""
    g = lambda t: t.to(torch.float64).clone().requires_grad_(requires_grad)
    p = {k: g(sc[k]) for k in A.PARAMS}
    p["cf"] = g(sc["cf"]) if sc["cf"] is not None else None
    cam = (sc["view"], sc["proj"], sc["campos"], sc["tfx"], sc["tfy"], sc["H"], sc["W"])
    sf, op = filtered(p["s"], p["o"], f.to(torch.float64))
    if antialiasing:
        pre = RO.preprocess(p["m"], sf, p["q"], op, p["sh"], p["cf"], *cam, deg)
        rho, _ = A.rho_from_conic(pre["conic"])
        op = op * rho
    out = RO.rasterize(p["m"], sf, p["q"], op, p["sh"], p["cf"], *cam, sc["bg"], deg)
    return out, p


_cache = {}


def reference(shape, antialiasing):
    """The float64 render of `scene(shape)` with its filter and the gradients of sum(wc colour) + sum(wd depth) + sum(wa alpha)
    (raster_aa_ref.loss_weights), for the activated parameters ("grads") and, by the activations' chain rule in float64, for the raw
    ones ("grads_raw": log-scales, a raw quaternion k q with the k of `raw_params`, logits).  Computed once; do not modify."""
    key = (shape, bool(antialiasing))
    if key not in _cache:
        sc, deg = scene(shape), shape[4]
        (oc, orad, od, oa, aux), p = rasterize(sc, deg, sc["f"], antialiasing, requires_grad=True)
        wc, wd, wa = A.loss_weights(sc["H"], sc["W"])
        ((oc * wc).sum() + (od * wd).sum() + (oa * wa).sum()).backward()
        grads = {k: p[k].grad.clone() for k in A.PARAMS}
        if sc["cf"] is not None:
            grads["cf"] = p["cf"].grad.clone()
        raw = raw_params(sc)
        qn = sc["q"] / sc["q"].norm(dim=1, keepdim=True)
        gq = grads["q"]
        graw = dict(grads)
        graw["s"] = grads["s"] * sc["s"]
        graw["o"] = grads["o"] * sc["o"] * (1.0 - sc["o"])
        graw["q"] = (gq - qn * (qn * gq).sum(1, keepdim=True)) / raw["q"].norm(dim=1, keepdim=True)
        _cache[key] = dict(sc=sc, deg=deg, color=oc.detach(), depth=od.detach(), alpha=oa.detach(), radii=orad, grads=grads,
                           grads_raw=graw, valid=aux["pre"]["valid"], weights=(wc, wd, wa))
    return _cache[key]


def raw_params(sc):
    """The trainer's parameters of a scene: log-scales, unnormalised quaternions k q (k in [0.5, 2], seeded), opacity logits."""
    g = torch.Generator().manual_seed(17)
    k = 0.5 + 1.5 * torch.rand(sc["q"].shape[0], 1, generator=g, dtype=torch.float64)
    return dict(s=torch.log(sc["s"]), q=sc["q"] * k, o=torch.log(sc["o"] / (1.0 - sc["o"])))


# ---- the property: a Gaussian far below the training views' sampling rate, seen from close by
PROP = dict(scale=1e-3, z_train=2.0, z_close=0.25, H=64, W=64, blend_opacity=0.95)


def property_scene():
    """One isotropic Gaussian of scale 1e-3 on the axis at z = 2 of a 64 x 64 training camera (60 degree fov), and the camera that
    looks at it from z = 0.25 (eye at z = 1.75).  Its filter is sqrt(0.2) 2 / fx = 0.0161 and coef = (s^2 / (s^2 + f^2))^1.5 =
    2.4e-4: under an opacity <= 1 the filtered Gaussian stays below the blend's 1/255 cut and NOTHING is drawn - the method keeps
    the 3D energy.  The test is about the SHAPE, so the (activated-route) opacity is blend_opacity / coef, coef from the closed form
    in float64: the blend multiplies 0.95 at the centre.  -> (scene dict seen from close by, filter [1], fx, coef)"""
    H, W = PROP["H"], PROP["W"]
    view0, _, _, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float64)
    m = torch.tensor([[0.0, 0.0, PROP["z_train"]]], dtype=torch.float64)
    f = filter_reference(m, camera_row(view0, tfx, tfy, H, W)[None])["filter"]
    s = torch.full((1, 3), PROP["scale"], dtype=torch.float64)
    coef = float((PROP["scale"] ** 2 / (PROP["scale"] ** 2 + float(f[0]) ** 2)) ** 1.5)
    view, proj, campos, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float64, eye=(0.0, 0.0, PROP["z_train"] - PROP["z_close"]))
    sh = torch.zeros(1, 16, 3, dtype=torch.float64)
    sh[:, 0] = 1.0
    sc = dict(m=m, s=s, q=torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64),
              o=torch.tensor([PROP["blend_opacity"] / coef], dtype=torch.float64), sh=sh, cf=None, view=view, proj=proj, campos=campos,
              tfx=tfx, tfy=tfy, bg=torch.zeros(3, dtype=torch.float64), H=H, W=W, N=1)
    return sc, f, W / (2.0 * tfx), coef


def second_moment(alpha):
    """per-axis second moment (px^2) of an alpha image [1,H,W] about its own centroid: sum a ((x - cx)^2 + (y - cy)^2) / (2 sum a)"""
    a = alpha.detach().to("cpu", torch.float64)[0]
    H, W = a.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    tot = a.sum()
    cx, cy = (a * xs).sum() / tot, (a * ys).sum() / tot
    return float((a * ((xs - cx) ** 2 + (ys - cy) ** 2)).sum() / (2.0 * tot))
