"""float64 reference of the rasteriser's PROJECTION stage (k_preprocess, k_preprocess_bwd with sh_backward, and the shared ewa_rows /
ewa_cov / mip_* / f3d_scales of csrc/raster_common.h), per Gaussian: the scenes, the reference, the error measure, the bars and the
mutants.  A plain module, not collected; tests/test_raster_proj_cpu.py checks everything said here about the scenes and that the
mutants are caught, tests/test_raster_proj_gpu.py holds the kernels to it.

The reference is oracle/raster_oracle.py (`preprocess`, `build_tile_lists`, `render`: the three calls of its `rasterize`) under the
float64 compositions the modes already have: `raster_aa_ref.rho_from_conic`, `raster_f3d_ref.filtered` and the raw route's chain rule
of `raster_f3d_ref.reference`.  `scale_modifier` is the oracle's own argument; with F3D it multiplies the FILTERED scales and coef
comes from the unmodified ones, as k_preprocess has it.  Every scene tensor (the camera too) is rounded to float32 and back before
the reference sees it: input rounding is no part of an error.

The measure, for group k in GROUPS and Gaussian i:
    rel[k][i] = max |got - ref| over the entries of Gaussian i in group k  /  max |ref| over the same entries
one bar per Gaussian and group where the older gradient tests have one per tensor (under which a Gaussian whose gradient is 1 % of
the scene's largest may be wrong by 20 % of itself).  Where the reference's entries are all exactly zero (the SH gradient of a
Gaussian whose three colour channels are clamped) the measure is 0 if the kernel's are too and infinite otherwise.

Mutants (`MUTANTS`): subtly wrong projections, each ONE textual patch of the oracle's source (asserted to apply exactly once), or one
switch in the compositions of this file - never a patch of the kernels."""
import inspect
import math

import numpy as np
import torch

import raster_aa_ref as A
import raster_f3d_ref as F
from oracle import raster_oracle as RO

H, W = 96, 112
GROUPS = ("m", "s", "q", "o", "sh", "cf", "m2")
MODES = {"plain": (False, False), "aa": (True, False), "f3d": (False, True), "f3d_aa": (True, True)}      # (antialiasing, filter3d)
RADIUS_EDGE = F.RADIUS_EDGE
D64 = torch.float64

# Per-Gaussian bars of the gradients, per scene family and group: <= 2 x the worst value measured on an MI355X (the module docstring
# of tests/test_raster_proj_gpu.py has the measurements and where each worst case sits).
#   "lattice"  the lattice under the four modes, with and without confidence, on both routes, the scale modifiers, the clamp scene
#   "layouts"  the lattice under every (degree, coefficients) pair: at degree 0 under the colour-only loss the screen-space sums of a
#              Gaussian cancel further than anywhere else (a constant colour against a background of other sign per channel)
#   "guard"    one large Gaussian in or next to the guard band
#   "blocks"   lattice Gaussians among culled ones
#   "near"     the point-like Gaussians of the near-plane scene, where den2inv = 1 / (den^2 + 1e-7) is the published regulariser and
#              not the analytic derivative: at cov2D + 0.3 I = 0.3 I it shifts the covariance-path gradient (s, q, and m through dT)
#              by up to 1e-7 / 0.09^2 = 1.2e-5 of itself - what s and q measure (1.27e-5) - on top of the rounding
# "q_raw": the raw route's quaternion gradient, (g - q (q . g)) / |q_raw|: the radial part of g that the projection takes out is 2 to
# 29 times what is left (tests/test_raster_proj_cpu.py prints it for the mutant that omits the projection), so the fp32 difference
# carries that many times the rounding of the activated route's gradient.
BAR = {
    "lattice": {"m": 1.9e-05, "s": 2.7e-06, "q": 3.1e-06, "q_raw": 5.1e-05, "o": 3.1e-06, "sh": 1.5e-06, "cf": 3e-06, "m2": 2.1e-05},
    "layouts": {"m": 7.3e-05, "s": 1.1e-05, "q": 1.4e-05, "o": 1.2e-05, "sh": 1e-06, "cf": 1.2e-05, "m2": 7.1e-05},
    "guard": {"m": 3.1e-06, "s": 2.6e-06, "q": 3.3e-06, "q_raw": 1.6e-05, "o": 3.4e-06, "sh": 3.3e-06, "cf": 3.4e-06, "m2": 3.1e-06},
    "blocks": {"m": 4.8e-06, "s": 1.7e-06, "q": 2.9e-06, "o": 2.6e-06, "sh": 1e-06, "cf": 2.7e-06, "m2": 5.7e-06},
    "near": {"m": 3.7e-05, "s": 2.5e-05, "q": 2.5e-05, "o": 1.6e-06, "sh": 1.1e-06, "cf": 1.5e-06, "m2": 2.7e-05},
}
# The forward's per-Gaussian state, from the arithmetic (eps = 2^-23 = 1.2e-7), not from a measurement:
#   depth          relative; three fused multiply-adds                                                                  8 eps
#   means2D        absolute, pixels: ndc through a 4-term dot product, + 1e-7, a reciprocal and a product (about 4 eps |ndc|, |ndc| <=
#                  1.5 W / 2 pixels each) and ndc2pix (2 eps |px|, |px| <= 140): 4e-5 + 3.4e-5                          1e-4 px
#   cov3D          relative to the Gaussian's largest entry: R from quaternion products (4 roundings), times s, three products summed 32 eps
#   conic          relative to its largest entry: J W Sigma W^T J^T (about 30 roundings), then the 2 x 2 inverse, whose determinant
#                  cancels by the condition number of cov2D (<= 6 here)                                                  2e-5
#   rgb            absolute: 16 terms of at most 1 in magnitude, a few roundings each                                   1e-5
#   blend_opacity  relative: op coef rho cf, coef from three divisions and square roots, rho from the ratio of two determinants 2e-5
#   opacity        relative: the input itself (exact, asserted) or the raw route's sigmoid                               8 eps
EPS32 = 2.0 ** -23
FWD_BAR = {"depth": 8 * EPS32, "means2D": 1e-4, "cov3D": 32 * EPS32, "conic": 2e-5, "rgb": 1e-5, "blend_opacity": 2e-5, "opacity": 8 * EPS32}


def r32(t):
    return t.to(torch.float32).to(D64)


def camera():
    view, proj, campos, tfx, tfy = RO.look_at_camera(H, W, dtype=D64)
    return dict(view=r32(view), proj=r32(proj), campos=r32(campos), tfx=float(np.float32(tfx)), tfy=float(np.float32(tfy)),
                bg=r32(torch.tensor([0.1, 0.3, 0.7], dtype=D64)), H=H, W=W)


def at_pixel(px, py, z, cam):
    """world position (the camera sits at the origin and looks down +z) that projects to the pixel (px, py) at depth z"""
    x = ((2.0 * px + 1.0) / W - 1.0) * cam["tfx"] * z
    y = ((2.0 * py + 1.0) / H - 1.0) * cam["tfy"] * z
    return torch.stack([x, y, z], 1)


def _finish(name, cam, m, s, q, o, sh, cf, f):
    sc = dict(cam)
    sc.update(name=name, N=m.shape[0], m=r32(m), s=r32(s), q=r32(q), o=r32(o), sh=r32(sh), cf=r32(cf), f=r32(f))
    return sc


# Chosen by search over seeds 1 .. 80 (tests/test_raster_proj_cpu.py asserts each property): in all four modes, with and without the
# confidence, the lattice is isolated, no Gaussian sits on a radius edge and every one reaches alpha >= 1/255 on >= 30 pixels (a 3D
# filter of 3 x the scale takes coef to 0.03: at other seeds some Gaussian is never drawn); the largest radius is 10 without the 3D
# filter and every per-Gaussian denominator of the full loss is >= 0.9 there.
LATTICE_SEED = 63
GRID0, PITCH, COLS, ROWS = 12, 24, 5, 4


def lattice(seed=LATTICE_SEED):
    """20 Gaussians within +-0.5 px of a 24-px grid from (12, 12): depth 2.5 - 5.5, sigma 1 - 2.5 px with axis ratios 0.6 - 1.4, random
    unit quaternions, opacity 0.3 - 0.9, SH 0.3 N(0,1) (16 coefficients), confidence 0.2 - 1, and a 3D filter of 0.3 - 3 x the mean
    scale that is exactly 0 for Gaussians 3 and 11."""
    cam = camera()
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=D64)
    n = COLS * ROWS
    i = torch.arange(n)
    px = GRID0 + PITCH * (i % COLS) + (u(n) - 0.5)
    py = GRID0 + PITCH * (i // COLS) + (u(n) - 0.5)
    z = 2.5 + 3.0 * u(n)
    fx = W / (2.0 * cam["tfx"])
    s = ((1.0 + 1.5 * u(n)) * z / fx)[:, None] * (0.6 + 0.8 * u(n, 3))
    q = torch.randn(n, 4, generator=g, dtype=D64)
    q = q / q.norm(dim=1, keepdim=True)
    o = 0.3 + 0.6 * u(n)
    sh = 0.3 * torch.randn(n, 16, 3, generator=g, dtype=D64)
    cf = 0.2 + 0.8 * u(n)
    f = (0.3 + 2.7 * u(n)) * s.mean(1)
    f[3] = f[11] = 0.0
    return _finish("lattice", cam, at_pixel(px, py, z, cam), s, q, o, sh, cf, f)


def take(sc, idx, name):
    out = dict(sc)
    for k in ("m", "s", "q", "o", "sh", "cf", "f"):
        out[k] = sc[k][idx].clone()
    out.update(N=len(idx), name=name)
    return out


# ---- guard: t.x / t.z (t.y / t.z) as multiples of tan(fovx) (tan(fovy)); the band ends at 1.3
GUARD = {"x+": (1.45, 0.1), "x-": (-1.45, -0.1), "y+": (0.1, 1.5), "y-": (-0.1, -1.5), "corner": (1.45, 1.5),
         "ctl_x": (1.25, 0.1), "ctl_y": (0.1, 1.25)}


def guard(which, seed=5):
    """ONE large Gaussian (sigma about 9 px at z = 3, axis ratios 1 : 0.8 : 1.2, opacity 0.8) whose centre lies off the image, in or
    beyond the guard band of ewa_rows; its footprint reaches into the image."""
    cam = camera()
    ax, ay = GUARD[which]
    g = torch.Generator().manual_seed(seed + sorted(GUARD).index(which))
    z = 3.0
    m = torch.tensor([[ax * cam["tfx"] * z, ay * cam["tfy"] * z, z]], dtype=D64)
    fx = W / (2.0 * cam["tfx"])
    s = (9.0 * z / fx) * torch.tensor([[1.0, 0.8, 1.2]], dtype=D64)
    q = torch.randn(1, 4, generator=g, dtype=D64)
    q = q / q.norm(dim=1, keepdim=True)
    sh = 0.3 * torch.randn(1, 16, 3, generator=g, dtype=D64)
    cf = 0.2 + 0.8 * torch.rand(1, generator=g, dtype=D64)
    f = (0.3 + 2.7 * torch.rand(1, generator=g, dtype=D64)) * s.mean(1)
    return _finish("guard_" + which, cam, m, s, q, torch.tensor([0.8], dtype=D64), sh, cf, f)


def clamp_scene():
    """lattice Gaussians 0 .. 7 with the DC coefficients set so that Gaussian k's clamp mask is k: a clamped channel's colour before
    the clamp is -0.2, an unclamped one's 0.6"""
    sc = take(lattice(), list(range(8)), "clamp")
    dirs = sc["m"] - sc["campos"][None]
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    sh = sc["sh"].clone()
    sh[:, 0] = 0.0
    rest = RO.eval_sh(3, sh, dirs)
    target = torch.tensor([[-0.2 if (k >> c) & 1 else 0.6 for c in range(3)] for k in range(8)], dtype=D64)
    sh[:, 0] = (target - 0.5 - rest) / RO.SH_C0
    sc["sh"] = r32(sh)
    return sc


BLOCK_N = (1, 255, 256, 257, 513)
BLOCK_SLOTS = (0, 254, 255, 256, 257, 511, 512)
CULL_KINDS = ("behind", "near", "off_axis", "off_edge")


def blocks(N):
    """N Gaussians: lattice Gaussians at the indices BLOCK_SLOTS and N - 1 (where they exist), every other index a culled one, cycling
    through: behind the camera (z = -1), t.z = 0.19, x = 40 (far off axis), and a small Gaussian 8 px left of the image whose tile
    rectangle is empty although it lies inside the guard band.  (det == 0 cannot be built: the dilation keeps det(cov2D + 0.3 I)
    >= 0.09 for every finite input.)"""
    lat = lattice()
    slots = sorted({i for i in BLOCK_SLOTS + (N - 1,) if i < N})
    cam = camera()
    fx = W / (2.0 * cam["tfx"])
    base = take(lat, [0] * N, f"blocks{N}")
    kind = []
    for i in range(N):
        if i in slots:
            j = slots.index(i)
            for k in ("m", "s", "q", "o", "sh", "cf", "f"):
                base[k][i] = lat[k][j]
            kind.append("visible")
            continue
        c = CULL_KINDS[len([x for x in kind if x != "visible"]) % 4]
        kind.append(c)
        z = 3.0
        if c == "behind":
            base["m"][i] = torch.tensor([0.1, 0.1, -1.0], dtype=D64)
        elif c == "near":
            base["m"][i] = torch.tensor([0.01, 0.01, 0.19], dtype=D64)
        elif c == "off_axis":
            base["m"][i] = torch.tensor([40.0, 0.2, z], dtype=D64)
        else:
            base["m"][i] = at_pixel(torch.tensor([-8.0], dtype=D64), torch.tensor([40.0], dtype=D64), torch.tensor([z], dtype=D64), cam)[0]
            base["s"][i] = 0.5 * z / fx
    for k in ("m", "s"):
        base[k] = r32(base[k])
    base["kind"], base["slots"] = kind, slots
    return base


NEAR_EPS = 1e-3


def near_scene():
    """Point-like Gaussians (scales 1e-4 (1, 0.5, 2): at most 0.1 px on screen, cov2D + 0.3 I = 0.3 I to 3 %; unequal, so that the
    rotation has a gradient) next to the near plane, each at its own lattice site: four pairs at t.z = 0.2 (1 -+ 1e-3) -
    the near one (even index) is culled, the far one (odd index) visible - and Gaussian 8 at EXACTLY float32(0.2), culled by
    `t.z <= kNearClip`.  The view matrix is the identity, so t.z is the mean's z to the bit."""
    lat = lattice()
    sc = take(lat, list(range(9)), "near")
    cam = camera()
    zs = [0.2 * (1 - NEAR_EPS), 0.2 * (1 + NEAR_EPS)] * 4 + [float(np.float32(0.2))]
    z = r32(torch.tensor(zs, dtype=D64))
    i = torch.arange(9)
    px = (GRID0 + PITCH * (i % COLS)).to(D64) + 0.3
    py = (GRID0 + PITCH * (i // COLS)).to(D64) - 0.2
    sc["m"] = r32(at_pixel(px, py, z, cam))
    sc["m"][:, 2] = z
    sc["s"] = r32(torch.full((9, 3), 1e-4, dtype=D64) * torch.tensor([1.0, 0.5, 2.0], dtype=D64))
    sc["f"] = r32(2.0 * sc["s"].mean(1))
    return sc


def with_modifier(sc, sm):
    """the scene whose render under scale_modifier = sm is `sc`'s under 1: scales and filter divided by sm (then rounded to float32)"""
    out = dict(sc)
    out["s"], out["f"], out["name"] = r32(sc["s"] / sm), r32(sc["f"] / sm), f"{sc['name']}_sm{sm}"
    return out


SH_LAYOUTS = ((0, 1), (0, 16), (1, 4), (1, 16), (2, 9), (2, 16), (3, 16))


def with_coeffs(sc, M):
    out = dict(sc)
    out["sh"], out["name"] = sc["sh"][:, :M].clone(), f"{sc['name']}_M{M}"
    return out


RAW_NORMS = (1e-3, 0.5, 2.0, 1e3)


def raw_params(sc, k=None):
    """the trainer's parameters of `sc`, rounded to float32: raster_f3d_ref.raw_params (quaternion norms in [0.5, 2]), or every
    quaternion scaled to the norm `k`"""
    p = F.raw_params(sc)
    if k is not None:
        p["q"] = sc["q"] / sc["q"].norm(dim=1, keepdim=True) * k
    return {n: r32(t) for n, t in p.items()}


# ------------------------------------------------------------------------------------------------------------------ loss
def loss_weights(loss):
    """"full": sum(colour ramp (1, -0.7, 0.45)) + 0.6 sum(depth ramp) + 0.8 sum(alpha ramp), ramp = 1 + 0.5 sin(0.11 x + 0.07 y) -
    smooth, so that one Gaussian's pixel sum does not cancel; "colour": the first term alone (the backward instance without
    dL_ddepth, which leaves G_DEPTH at zero).  -> (wc [3,H,W], wd [1,H,W] or None, wa or None), float32-exact values"""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=D64), torch.arange(W, dtype=D64), indexing="ij")
    ramp = r32(1.0 + 0.5 * torch.sin(0.11 * xs + 0.07 * ys))
    wc = r32(ramp[None] * torch.tensor([1.0, -0.7, 0.45], dtype=D64)[:, None, None])
    if loss == "colour":
        return wc, None, None
    assert loss == "full"
    return wc, r32(0.6 * ramp[None]), r32(0.8 * ramp[None])


# ------------------------------------------------------------------------------------------------------------------ mutants
def _st(value, grad_path):
    """`value` in the forward, the gradient of `grad_path` in the backward"""
    return value.detach() + grad_path - grad_path.detach()


class _ConicNoLowPassDen(torch.autograd.Function):
    """the conic of (a, b; b, c) (a, c dilated) with k_preprocess_bwd's backward formulas, `den` formed WITHOUT the low-pass"""
    @staticmethod
    def forward(ctx, a, b, c, low_pass_in_den):
        ctx.save_for_backward(a, b, c)
        ctx.lp = low_pass_in_den
        det = a * c - b * b
        return torch.stack([c / det, -b / det, a / det], 1)

    @staticmethod
    def backward(ctx, g):
        a, b, c = ctx.saved_tensors
        h = 0.0 if ctx.lp else 0.3
        den = (a - h) * (c - h) - b * b
        d2 = 1.0 / (den * den + 1e-7)
        gxx, gxy, gyy = g[:, 0], g[:, 1], g[:, 2]          # gxy: the gradient of the stored -b / det
        da = d2 * (-c * c * gxx + b * c * gxy + (den - a * c) * gyy)
        dc = d2 * ((den - a * c) * gxx + a * b * gxy - a * a * gyy)
        db = d2 * (2 * b * c * gxx - (den + 2 * b * b) * gxy + 2 * a * b * gyy)
        return da, db, dc, None


# name -> (function of the oracle that is patched, old text, new text); the patched `preprocess` sees `_st` and the class above
_PATCHES = {
    "guard_mul_omitted": ("preprocess", "(txtz.clamp(-limx, limx) * tz).detach(), t[:, 0])\n    ty = torch.where((tytz < -limy) | (tytz > limy), (tytz.clamp(-limy, limy) * tz).detach(), t[:, 1])",
                          "_st(txtz.clamp(-limx, limx) * tz, t[:, 0]), t[:, 0])\n    ty = torch.where((tytz < -limy) | (tytz > limy), _st(tytz.clamp(-limy, limy) * tz, t[:, 1]), t[:, 1])"),
    "guard_limit_1": ("preprocess", "limx, limy = 1.3 * tanfovx, 1.3 * tanfovy", "limx, limy = 1.0 * tanfovx, 1.0 * tanfovy"),
    "clamp_ignored": ("preprocess", "rgb = torch.clamp(rgb_raw, min=0.0)", "rgb = _st(torch.clamp(rgb_raw, min=0.0), rgb_raw)"),
    "clamp_rotated": ("preprocess", "rgb = torch.clamp(rgb_raw, min=0.0)",
                      "rgb = _st(torch.clamp(rgb_raw, min=0.0), rgb_raw * (~(rgb_raw < 0).roll(1, dims=1)))"),
    "modifier_not_in_dscale": ("preprocess", "Mm = R * (scale_modifier * scales)[:, None, :]",
                               "Mm = R * _st(scale_modifier * scales, scales)[:, None, :]"),
    "sh3_term_dropped": ("eval_sh", "SH_C3[1] * xy * z * sh[:, 10]", "SH_C3[1] * xy * z.detach() * sh[:, 10]"),
    "dsigma_offdiag_not_doubled": ("preprocess", "Sigma = Mm @ Mm.transpose(1, 2)\n",
                                   "Sigma = Mm @ Mm.transpose(1, 2)\n    Sigma = _st(Sigma, Sigma * (0.5 + 0.5 * torch.eye(3, dtype=dt)))\n"),
    "conf_not_in_dopacity": ("preprocess", "opacity=opacities * conf,", "opacity=_st(opacities * conf, opacities + opacities.detach() * conf),"),
    "lowpass_not_in_den": ("preprocess", "conic = torch.stack([c / det_safe, -b / det_safe, a / det_safe], 1)",
                           "conic = _ConicNoLowPassDen.apply(a, b, c, False)"),
    "near_lt": ("preprocess", "in_front = t[:, 2] > NEAR_CLIP", "in_front = t[:, 2] >= NEAR_CLIP"),
    # not a mutant: the class above with the low-pass IN den is the oracle's own derivative (tests/test_raster_proj_cpu.py checks it)
    "_conic_formulas": ("preprocess", "conic = torch.stack([c / det_safe, -b / det_safe, a / det_safe], 1)",
                        "conic = _ConicNoLowPassDen.apply(a, b, c, True)"),
}
# ... and the switches in this file's own compositions
_SWITCHES = ("modifier_in_coef", "raw_quat_not_projected")
MUTANTS = ("guard_mul_omitted", "guard_limit_1", "clamp_ignored", "clamp_rotated", "modifier_not_in_dscale", "modifier_in_coef",
           "sh3_term_dropped", "dsigma_offdiag_not_doubled", "raw_quat_not_projected", "conf_not_in_dopacity", "lowpass_not_in_den",
           "near_lt")


def patched_preprocess(mutant):
    """oracle.raster_oracle.preprocess with the one patch of `mutant` (None, or a switch of this file: the function itself)"""
    if mutant is None or mutant in _SWITCHES:
        return RO.preprocess
    fn, old, new = _PATCHES[mutant]
    src = inspect.getsource(getattr(RO, fn))
    assert src.count(old) == 1, f"mutant {mutant}: the text it patches occurs {src.count(old)} times in oracle.raster_oracle.{fn}"
    ns = dict(vars(RO))
    ns.update(_st=_st, _ConicNoLowPassDen=_ConicNoLowPassDen)
    exec(compile(src.replace(old, new), f"<{mutant}>", "exec"), ns)
    if fn != "preprocess":                      # preprocess looks the helper up in its globals: run it over the patched namespace
        exec(compile(inspect.getsource(RO.preprocess), f"<{mutant}>", "exec"), ns)
    return ns["preprocess"]


# ------------------------------------------------------------------------------------------------------------------ reference
_cache = {}


def reference(sc, deg, mode="plain", loss="full", sm=1.0, conf=True, raw=None, mutant=None, tag=None):
    """The float64 projection state and gradients of scene `sc`.  `raw`: None, or the float32-rounded parameters of the raw route
    (`raw_params`), whose float64 activations then replace sc's s / q / o and whose gradients ("grads_raw") follow by the chain rule.
    `tag` names `raw` in the cache key.  Computed once per key; callers must not modify it.
    -> dict(valid, radius, tiles_touched, clamped, depth, means2D [N,2], cov3D [N,6], conic [N,3], rgb, opacity (plain), blend_opacity
            (op cf coef rho), grads {group: tensor}, grads_raw {s, q, o} or None, lam_arg (3 sqrt(lambda): the radius before ceil),
            px_alpha: per Gaussian the [H,W] bool map of the pixels where its alpha reaches 1/255)"""
    key = (sc["name"], deg, mode, loss, sm, conf, ("raw", tag) if raw is not None else None, mutant)
    if key in _cache:
        return _cache[key]
    aa, f3d = MODES[mode]
    leaf = lambda t: t.to(D64).clone().requires_grad_(True)
    s_in, q_in, o_in = sc["s"], sc["q"], sc["o"]
    if raw is not None:
        s_in, q_in, o_in = torch.exp(raw["s"]), raw["q"] / raw["q"].norm(dim=1, keepdim=True), torch.sigmoid(raw["o"])
    p = dict(m=leaf(sc["m"]), s=leaf(s_in), q=leaf(q_in), o=leaf(o_in), sh=leaf(sc["sh"]))
    p["cf"] = leaf(sc["cf"]) if conf else None
    cam = (sc["view"], sc["proj"], sc["campos"], sc["tfx"], sc["tfy"], H, W)
    pre_fn = patched_preprocess(mutant)
    s_eff, o_eff = p["s"], p["o"]
    if f3d:
        s_eff, o_eff = F.filtered(p["s"], p["o"], sc["f"])
        if mutant == "modifier_in_coef":
            o_eff = p["o"] * (sm * p["s"] / torch.sqrt((sm * p["s"]) ** 2 + (sc["f"] ** 2)[:, None])).prod(dim=1)
    if aa:
        rho, _ = A.rho_from_conic(pre_fn(p["m"], s_eff, p["q"], o_eff, p["sh"], p["cf"], *cam, deg, sm)["conic"])
        o_eff = o_eff * rho
    pre = pre_fn(p["m"], s_eff, p["q"], o_eff, p["sh"], p["cf"], *cam, deg, sm)
    _, plist, ranges = RO.build_tile_lists(pre)
    pre["px"].retain_grad()
    pre["py"].retain_grad()
    color, depth, alpha, _ = RO.render(pre, plist, ranges, sc["bg"], H, W)
    wc, wd, wa = loss_weights(loss)
    L = (color * wc).sum()
    if wd is not None:
        L = L + (depth * wd).sum() + (alpha * wa).sum()
    L.backward()
    valid = pre["valid"]
    z = lambda g, like: (torch.zeros_like(like) if g is None else g).detach() * valid.reshape(-1, *[1] * (like.dim() - 1))
    grads = {k: z(p[k].grad, p[k]) for k in ("m", "s", "q", "o", "sh")}
    if conf:
        grads["cf"] = z(p["cf"].grad, p["cf"])
    grads["m2"] = torch.stack([0.5 * W * z(pre["px"].grad, pre["px"]), 0.5 * H * z(pre["py"].grad, pre["py"])], 1)
    graw = None
    if raw is not None:
        qn, gq = q_in, grads["q"]
        proj = gq if mutant == "raw_quat_not_projected" else gq - qn * (qn * gq).sum(1, keepdim=True)
        graw = dict(s=grads["s"] * s_in, o=grads["o"] * o_in * (1.0 - o_in), q=proj / raw["q"].norm(dim=1, keepdim=True))
    with torch.no_grad():
        Sig = RO.quat_to_rot(p["q"]) * (sm * s_eff)[:, None, :]
        Sig = Sig @ Sig.transpose(1, 2)
        cov3D = torch.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], 1)
        conic = pre["conic"].detach()
        ys, xs = torch.meshgrid(torch.arange(H, dtype=D64), torch.arange(W, dtype=D64), indexing="ij")
        dx, dy = pre["px"].detach()[:, None, None] - xs[None], pre["py"].detach()[:, None, None] - ys[None]
        power = -0.5 * (conic[:, 0, None, None] * dx * dx + conic[:, 2, None, None] * dy * dy) - conic[:, 1, None, None] * dx * dy
        a_px = torch.clamp(pre["opacity"].detach()[:, None, None] * torch.exp(power), max=0.99)
        px_alpha = (a_px >= 1.0 / 255.0) & (power <= 0) & valid[:, None, None]
    out = dict(valid=valid, radius=pre["radius"], tiles_touched=pre["tiles_touched"],
               clamped=(pre["clamped"].to(torch.int64) * torch.tensor([1, 2, 4])).sum(1), depth=pre["depth"].detach(),
               means2D=torch.stack([pre["px"], pre["py"]], 1).detach(), cov3D=cov3D, conic=conic, rgb=pre["rgb"].detach(),
               opacity=p["o"].detach(), blend_opacity=pre["opacity"].detach(), grads=grads, grads_raw=graw,
               lam_arg=3.0 * torch.sqrt(F.lam_max(conic)), px_alpha=px_alpha, t=(torch.cat([p["m"].detach(), torch.ones(sc["N"], 1, dtype=D64)], 1)
                                                                               @ sc["view"])[:, :3])
    _cache[key] = out
    return out


# ------------------------------------------------------------------------------------------------------------------ measure
def entries(group, t):
    """the entries of a gradient tensor that belong to the measure: all, but the two screen axes of dL_dmeans2D"""
    t = t.detach().to("cpu", D64)
    return (t[:, :2] if group == "m2" else t).reshape(t.shape[0], -1)


def per_gaussian(group, got, ref):
    """-> (rel [N], den [N]): the measure of the module docstring for every Gaussian (0 / 0 = 0, x / 0 = inf)"""
    g, r = entries(group, got), entries(group, ref)
    assert g.shape == r.shape, (group, g.shape, r.shape)
    num, den = (g - r).abs().amax(1), r.abs().amax(1)
    rel = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, math.inf), torch.zeros_like(num)))
    return rel, den


def global_measure(got, ref):
    """the older tests' measure (tests/test_raster_gpu.py::test_backward_vs_autograd): max |got - ref| / max |ref| over a tensor"""
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def isolated(ref):
    """no pixel at which two Gaussians' alphas both reach 1/255"""
    return int(ref["px_alpha"].sum(0).max()) <= 1


def radius_edges(ref):
    """visible Gaussians whose 3 sqrt(lambda) lies within RADIUS_EDGE of an integer (an fp32 radius may land on the other side)"""
    arg = ref["lam_arg"]
    return int((ref["valid"] & ((arg - torch.round(arg)).abs() < RADIUS_EDGE)).sum())


def mixed_scene():
    """What the older gradient tests render - a random mid-frustum field (tests/test_raster_gpu.py's recipe: 300 Gaussians, 5 behind
    the camera, 5 at x = 40) - plus the guard-band Gaussian "x+", the clamp scene's eight and the lattice's first four."""
    cam = camera()
    m, s, q, o, sh = RO.synthetic_gaussians(300, seed=300 + H, dtype=D64, log_scale_mean=np.log(0.02))
    m[:5, 2] = -1.0
    m[5:10, 0] = 40.0
    g = torch.Generator().manual_seed(4)
    cf = 0.2 + 0.8 * torch.rand(300, generator=g, dtype=D64)
    field = _finish("field", cam, m, s, q, o, sh, cf, s.mean(1))
    parts = [field, guard("x+"), clamp_scene(), take(lattice(), [8, 9, 10, 11], "l4")]
    out = dict(cam)
    for k in ("m", "s", "q", "o", "sh", "cf", "f"):
        out[k] = torch.cat([pt[k] for pt in parts])
    out.update(name="mixed", N=out["m"].shape[0])
    return out
