"""The blend backward's algebraic forms (csrc/raster_bwd.hip) against float64 autograd through oracle/raster_oracle.py.

k_render_bwd carries ONE running scalar R per pixel for everything behind the current splat (instead of four colour / depth
recursions), sums raw moments of h = G * dL/dalpha per (tile, splat) and leaves the per-Gaussian factors (opacity, conic,
W/2, H/2) to k_preprocess_bwd, and has an instance without the depth-gradient terms.  The scenes below are small and built
so that each place where those forms can go wrong is present - and asserted present:
  * tile lists longer than one staging round (128) and than two (256): R, like T, is carried across rounds;
  * image sizes that are no multiple of 16, partial tiles in the upper half-tile (53 rows) and in the lower (45 rows);
  * a stack deep enough that some pixels saturate (T < 1e-4) before the end of their list while others never do;
  * layers at the 0.99 alpha clamp in front of translucent ones;
  * a non-zero background, and a per-Gaussian confidence (the opacity the blend multiplied is opacity x confidence).
Every scene runs with four losses: colour, colour + depth, colour + alpha, all three - the two template instances of the
kernel (with / without a depth gradient) times the alpha-output term of `tail`.
Bar: 2e-3 of the group's largest gradient, the project's bar for small scenes (test_raster_gpu.py), all groups, no case left out."""
import numpy as np
import pytest
import torch

from oracle import raster_oracle as RO

pytestmark = pytest.mark.gpu

LOSSES = {"colour": (1, 0, 0), "colour+depth": (1, 1, 0), "colour+alpha": (1, 0, 1), "colour+depth+alpha": (1, 1, 1)}
SCENES = ("rows53", "rows45")
FOVX = 60.0


def _at_pixel(u, v, z, H, W):
    """world (x, y) that projects to pixel centre (u, v) at depth z for look_at_camera(H, W)"""
    f = W / (2.0 * np.tan(np.deg2rad(FOVX) / 2))
    return (u - 0.5 * (W - 1)) * z / f, (v - 0.5 * (H - 1)) * z / f


def _cluster(g, n, u, v, jitter, sigma_px, opacity, H, W, zr=(3.0, 4.0)):
    dt = torch.float64
    f = W / (2.0 * np.tan(np.deg2rad(FOVX) / 2))
    z = zr[0] + (zr[1] - zr[0]) * torch.rand(n, generator=g, dtype=dt)
    uu = u + jitter * (2 * torch.rand(n, generator=g, dtype=dt) - 1)
    vv = v + jitter * (2 * torch.rand(n, generator=g, dtype=dt) - 1)
    m = torch.stack([(uu - 0.5 * (W - 1)) * z / f, (vv - 0.5 * (H - 1)) * z / f, z], 1)
    s = (sigma_px * z / f)[:, None] * (0.8 + 0.4 * torch.rand(n, 3, generator=g, dtype=dt))
    q = torch.randn(n, 4, generator=g, dtype=dt)
    q = q / q.norm(dim=1, keepdim=True)
    o = opacity * (0.7 + 0.3 * torch.rand(n, generator=g, dtype=dt))
    sh = 0.3 * torch.randn(n, 16, 3, generator=g, dtype=dt)
    return m, s, q, o, sh


def build_scene(name):
    """A sparse random field, a deep cluster (> 256 entries in one tile, saturating in its middle), a second cluster
    (> 128 entries) behind an opaque layer, and three opacity-1 Gaussians centred ON pixel centres (alpha clamps at 0.99)."""
    dt = torch.float64
    if name == "rows53":         # 53 = 3 * 16 + 5: the last tile row has 5 rows, all in the upper half-tile; 75 = 4 * 16 + 11
        H, W, seed, conf = 53, 75, 11, False
        deep_uv, mid_uv = (40.0, 24.0), (69.0, 50.0)     # on the border of the two half-tiles / in the ragged corner tile
        clamp_uv = [(12, 12), (52, 40), (69, 50)]
    else:                        # 45 = 2 * 16 + 13: the last tile row has 5 rows in its LOWER half-tile; 70 = 4 * 16 + 6
        H, W, seed, conf = 45, 70, 23, True
        deep_uv, mid_uv = (66.0, 40.0), (20.0, 10.0)     # in the ragged corner tile, across its half-tile border
        clamp_uv = [(50, 8), (10, 38), (20, 10)]
    g = torch.Generator().manual_seed(seed)
    parts = [RO.synthetic_gaussians(500, seed=seed, dtype=dt, log_scale_mean=np.log(0.06), zrange=(2.5, 6.0))]
    parts.append(_cluster(g, 420, *deep_uv, 2.5, 0.8, 0.7, H, W))
    parts.append(_cluster(g, 170, *mid_uv, 2.0, 0.8, 0.06, H, W))
    cm, cs, cq, co, csh = _cluster(g, len(clamp_uv), 0.0, 0.0, 0.0, 9.0, 1.0, H, W, zr=(2.1, 2.2))
    for k, (u, v) in enumerate(clamp_uv):
        x, y = _at_pixel(u, v, float(cm[k, 2]), H, W)
        cm[k, 0], cm[k, 1] = x, y
    cs[:] = cs.mean(1, keepdim=True)             # isotropic: the footprint's peak is the pixel centre itself
    co[:] = 1.0
    parts.append((cm, cs, cq, co, csh))
    m, s, q, o, sh = (torch.cat([p[i] for p in parts], 0) for i in range(5))
    N = m.shape[0]
    clamp_ids = list(range(N - len(clamp_uv), N))
    cf = None
    if conf:
        cf = 0.5 + 0.5 * torch.rand(N, generator=g, dtype=dt)
        cf[clamp_ids] = 1.0
    view, proj, campos, tfx, tfy = RO.look_at_camera(H, W, fovx_deg=FOVX, dtype=dt)
    bg = torch.tensor([0.2, 0.1, 0.4], dtype=dt)
    gw = torch.Generator().manual_seed(seed + 100)
    wc = torch.randn(3, H, W, generator=gw, dtype=dt)
    wd = 0.3 * torch.randn(1, H, W, generator=gw, dtype=dt)
    wa = torch.randn(1, H, W, generator=gw, dtype=dt)
    return dict(m=m, s=s, q=q, o=o, sh=sh, cf=cf, view=view, proj=proj, campos=campos, tfx=tfx, tfy=tfy, bg=bg, H=H, W=W,
                N=N, clamp_ids=clamp_ids, wc=wc, wd=wd, wa=wa)


def oracle_reference(sc):
    """float64 forward once, then the gradients of the four losses from the one graph.  Returns (aux, outputs, grads[loss])."""
    keys = ["m", "s", "q", "o", "sh"] + (["cf"] if sc["cf"] is not None else [])
    p = {k: sc[k].clone().requires_grad_(True) for k in keys}
    oc, _, od, oa, aux = RO.rasterize(p["m"], p["s"], p["q"], p["o"], p["sh"], p.get("cf"), sc["view"], sc["proj"],
                                      sc["campos"], sc["tfx"], sc["tfy"], sc["H"], sc["W"], sc["bg"], 3)
    pre = aux["pre"]
    grads = {}
    for name, (kc, kd, ka) in LOSSES.items():
        loss = kc * (oc * sc["wc"]).sum() + kd * (od * sc["wd"]).sum() + ka * (oa * sc["wa"]).sum()
        gs = torch.autograd.grad(loss, [p[k] for k in keys] + [pre["px"], pre["py"]], retain_graph=True)
        d = {k: g_.detach() for k, g_ in zip(keys, gs)}
        # means2D gradient as the published backward defines it: dL / d(NDC mean) = dL / d(pixel mean) * (W/2, H/2)
        d["m2"] = torch.stack([gs[-2].detach() * 0.5 * sc["W"], gs[-1].detach() * 0.5 * sc["H"]], 1)
        grads[name] = d
    return aux, (oc.detach(), od.detach(), oa.detach()), grads


def scene_features(sc, aux, outs):
    """What the scene exercises, from the oracle's own tile lists and per-pixel results."""
    H, W = sc["H"], sc["W"]
    gx = (W + 15) // 16
    ranges = aux["ranges"]
    length = ranges[:, 1] - ranges[:, 0]
    nc = aux["n_contrib"]
    ys, xs = np.mgrid[0:H, 0:W]
    tile_of = (ys // 16) * gx + xs // 16
    pre = aux["pre"]
    px, py, conic, op = (pre[k].detach().numpy() for k in ("px", "py", "conic", "opacity"))

    def raw_alpha(k, x, y):      # k: Gaussian ids [n], x / y: pixels [m] -> power, opacity * exp(power), both [n, m]
        dx, dy = px[k, None] - x[None], py[k, None] - y[None]
        power = -0.5 * (conic[k, 0, None] * dx * dx + conic[k, 2, None] * dy * dy) - conic[k, 1, None] * dx * dy
        return power, op[k, None] * np.exp(power)

    # a pixel saturated EARLY if a splat behind its last contributor would still have been taken (the forward stopped it at
    # T < 1e-4), and NEVER if nothing behind its last contributor reaches it
    early = never = 0
    for t in np.nonzero(length > 256)[0]:
        sel = tile_of == t
        ids = aux["point_list"][ranges[t, 0]:ranges[t, 1]]
        power, raw = raw_alpha(ids, xs[sel].astype(np.float64), ys[sel].astype(np.float64))
        ok = (power <= 0) & (np.minimum(raw, 0.99) >= 1.0 / 255.0)
        behind = (ok & (np.arange(1, len(ids) + 1)[:, None] > nc[sel][None])).any(0)
        early += int(behind.sum())
        never += int((~behind & (nc[sel] > 128)).sum())      # ... and it walked past a staging round to get there
    clamp_front = 0
    for k in sc["clamp_ids"]:
        _, raw = raw_alpha(np.array([k]), xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64))
        for y, x in zip(*np.nonzero(raw.reshape(H, W) > 0.99)):
            s_, e_ = ranges[tile_of[y, x]]
            idx = int(np.nonzero(aux["point_list"][s_:e_] == k)[0][0])
            clamp_front += int(nc[y, x] > idx + 1)           # the clamped layer was blended and so was a layer behind it
    return dict(longest=int(length.max()), one_to_two_rounds=int(((length > 128) & (length <= 256)).sum()),
                more_than_two_rounds=int((length > 256).sum()), early=early, never=never, clamp_front=clamp_front)


@pytest.fixture(scope="module")
def refs():
    out = {}
    for name in SCENES:
        sc = build_scene(name)
        aux, outs, grads = oracle_reference(sc)
        out[name] = (sc, aux, outs, grads)
    return out


def hip_grads(sc, dev, loss, zero_depth=False):
    """HIP forward + backward of one loss -> dict of float64 CPU gradients (the five groups, confidence, means2D)."""
    from syn3r_amd.raster import GaussianRasterizationSettings, GaussianRasterizer
    f = lambda t: t.to(dev, torch.float32).clone().requires_grad_(True)
    keys = ["m", "s", "q", "o", "sh"] + (["cf"] if sc["cf"] is not None else [])
    p = {k: f(sc[k]) for k in keys}
    m2 = torch.zeros(sc["N"], 3, device=dev, requires_grad=True)
    st = GaussianRasterizationSettings(sc["H"], sc["W"], sc["tfx"], sc["tfy"], sc["bg"].float().to(dev), 1.0,
                                       sc["view"].float().to(dev), sc["proj"].float().to(dev), 3,
                                       sc["campos"].float().to(dev), False, False)
    color, _, depth, alpha = GaussianRasterizer(st)(p["m"], m2, p["o"], shs=p["sh"], scales=p["s"], rotations=p["q"],
                                                    confidence=p.get("cf"))
    kc, kd, ka = LOSSES[loss]
    total = (color * sc["wc"].float().to(dev)).sum()
    if kd:
        total = total + (depth * sc["wd"].float().to(dev)).sum()
    if ka:
        total = total + (alpha * sc["wa"].float().to(dev)).sum()
    if zero_depth:                # an explicit all-zero depth gradient: the instance WITH the depth terms, fed zeros
        total = total + (depth * torch.zeros_like(depth)).sum()
    total.backward()
    out = {k: p[k].grad.detach().cpu().double() for k in keys}
    assert (m2.grad[:, 2] == 0).all()
    out["m2"] = m2.grad.detach().cpu().double()[:, :2]
    return out, (color.detach().cpu(), depth.detach().cpu(), alpha.detach().cpu())


def rel_diff(a, b):
    """per group: max |a - b| over the group's largest |b|"""
    return {k: float((a[k] - b[k]).abs().max()) / (float(b[k].abs().max()) + 1e-30) for k in b}


@pytest.mark.parametrize("name", SCENES)
def test_scene_has_what_it_is_for(name, refs):
    sc, aux, outs, _ = refs[name]
    ft = scene_features(sc, aux, outs)
    print(name, ft)
    assert sc["H"] % 16 != 0 and sc["W"] % 16 != 0 and sc["H"] <= 56 and sc["W"] <= 80
    assert (sc["H"] % 16 <= 8) == (name == "rows53")         # the partial tile row ends in the upper / in the lower half-tile
    assert ft["one_to_two_rounds"] >= 1 and ft["more_than_two_rounds"] >= 1, ft
    assert ft["early"] >= 8 and ft["never"] >= 8, ft
    assert ft["clamp_front"] >= 3, ft
    assert float(sc["bg"].abs().min()) > 0


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("name", SCENES)
def test_gradients_match_float64_autograd(name, loss, refs, gpu):
    sc, aux, outs, grads = refs[name]
    got, (color, depth, alpha) = hip_grads(sc, gpu, loss)
    np.testing.assert_allclose(color.numpy(), outs[0].numpy(), atol=3e-4)
    np.testing.assert_allclose(alpha.numpy(), outs[2].numpy(), atol=3e-4)
    err = rel_diff(got, grads[loss])
    print(name, loss, {k: f"{v:.2e}" for k, v in err.items()})
    assert set(err) >= {"m", "s", "q", "o", "sh", "m2"}
    for k, v in err.items():
        assert v < 2e-3, (name, loss, k, v)


# Two identical colour-only runs of the PARENT commit's kernels on scene "rows53" differ, through the order of the float atomics
# of Gaussians that span three or more tiles, by at most this fraction of a group's largest gradient: 2.504e-7 (group q; s 1.3e-7,
# sh 1.4e-7, m 3.7e-8, m2 2.9e-8, o 1.1e-9), the largest over all ordered pairs of 30 runs in each of 3 processes on MI355X.
# (This build, runs with and without the explicit zero mixed in the same way: 1.67e-7.  "rows45" gave ONE result bit for bit in
# all 90 runs of either build: no spread to scale, so the comparison runs on "rows53".)
RUN_TO_RUN = 2.504e-7
ZERO_DEPTH_BOUND = 4 * RUN_TO_RUN


def test_zero_depth_gradient_equals_none(refs, gpu):
    """No depth gradient (null pointer: the instance without the depth terms) against an explicit all-zero one (the instance
    with them): the same gradients up to the run-to-run spread of the atomics."""
    name = "rows53"
    sc = refs[name][0]
    a, _ = hip_grads(sc, gpu, "colour")
    b, _ = hip_grads(sc, gpu, "colour", zero_depth=True)
    err = rel_diff(b, a)
    print(name, {k: f"{v:.2e}" for k, v in err.items()})
    for k, v in err.items():
        assert v <= ZERO_DEPTH_BOUND, (name, k, v)
