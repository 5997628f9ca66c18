"""Every lane and every reduction slot of the blend backward (csrc/raster_bwd.hip) on its own, against float64 autograd.

k_render_bwd sums the contributions of a wavefront's 128 pixels to the ten gradient values of a splat across the lanes
(reduce_lanes: two swap levels, then DPP row rotates with bank masks that leave each total on ONE lane of a 16-lane row) and
adds the lanes' totals to the record slots reduce_value names.  A dense loss can hide a dropped lane, or a total that lands
in the wrong slot, under its bar: one pixel of 256 is a small part of a sum.  Here the colour gradient is ONE-HOT: one
backward pass per pixel, so the whole gradient of that pass comes from one lane (and one of its two pixels), and a
contribution that is lost or misplaced is off by the size of the gradient itself.

Scenes: one 16 x 16 tile (both wavefronts, every lane, both pixels of a lane) and a 16 x 13 image (the lower half-tile is
partial: rows 8-12, so the second pixel of rows 12-15's lanes does not exist).  Six rotated, anisotropic Gaussians (cxy != 0:
the xy moment is not zero by symmetry) with distinct depths and opacities 0.3 .. 0.9, wide enough that every one of them is
blended on every pixel - asserted from the oracle's per-pixel values - so every pass exercises all ten values of all six
splats.  Each pixel runs without a depth gradient (the kernel instance that sums nine values) and with a one-hot depth
gradient (the instance that sums ten).
Reference: float64 autograd through oracle/raster_oracle.py, one graph per scene.
Bar: 2e-3 of the group's largest gradient in that pass, the project's bar for small scenes (test_raster_gpu.py), every
parameter group and means2D, no pixel left out."""
import numpy as np
import pytest
import torch

from oracle import raster_oracle as RO

pytestmark = pytest.mark.gpu

SCENES = {"tile16x16": (16, 16), "rows13": (13, 16)}      # name -> (H, W)
FOVX = 60.0
N = 6
OPACITY = (0.30, 0.42, 0.55, 0.66, 0.78, 0.90)
W_COLOUR = (1.0, -0.7, 0.45)        # three different channel weights: a channel that lands in another's slot shows
W_DEPTH = 0.6
GROUPS = ("m", "s", "q", "o", "sh", "m2")
BAR = 2e-3


def build_scene(name):
    H, W = SCENES[name]
    dt = torch.float64
    g = torch.Generator().manual_seed(5 + H)
    f = W / (2.0 * np.tan(np.deg2rad(FOVX) / 2))
    z = torch.linspace(3.0, 4.0, N, dtype=dt)[torch.randperm(N, generator=g)]            # distinct depths, not in index order
    u = 0.5 * (W - 1) + 3.0 * (2 * torch.rand(N, generator=g, dtype=dt) - 1)
    v = 0.5 * (H - 1) + 3.0 * (2 * torch.rand(N, generator=g, dtype=dt) - 1)
    m = torch.stack([(u - 0.5 * (W - 1)) * z / f, (v - 0.5 * (H - 1)) * z / f, z], 1)
    sigma_px = 14.0
    s = (sigma_px * z / f)[:, None] * torch.tensor([[0.75, 1.0, 1.3]], dtype=dt)[:, torch.randperm(3, generator=g)]
    q = torch.randn(N, 4, generator=g, dtype=dt)
    q = q / q.norm(dim=1, keepdim=True)
    o = torch.tensor(OPACITY, dtype=dt)[torch.randperm(N, generator=g)]
    sh = 0.3 * torch.randn(N, 16, 3, generator=g, dtype=dt)
    sh[:, 0] = sh[:, 0].abs() + 0.3                  # colours well above the clamp at 0
    view, proj, campos, tfx, tfy = RO.look_at_camera(H, W, fovx_deg=FOVX, dtype=dt)
    bg = torch.tensor([0.2, 0.1, 0.4], dtype=dt)
    return dict(m=m, s=s, q=q, o=o, sh=sh, view=view, proj=proj, campos=campos, tfx=tfx, tfy=tfy, bg=bg, H=H, W=W)


def oracle_reference(sc):
    """float64 forward once; per pixel the gradients of the one-hot colour loss and of the one-hot depth loss (the backward is
    linear in the output gradient: the pass with both is their sum).  Returns (aux, colour[P][group], depth[P][group])."""
    keys = ["m", "s", "q", "o", "sh"]
    p = {k: sc[k].clone().requires_grad_(True) for k in keys}
    oc, _, od, _, aux = RO.rasterize(p["m"], p["s"], p["q"], p["o"], p["sh"], None, sc["view"], sc["proj"], sc["campos"],
                                     sc["tfx"], sc["tfy"], sc["H"], sc["W"], sc["bg"], 3)
    pre = aux["pre"]
    wrt = [p[k] for k in keys] + [pre["px"], pre["py"]]
    wc = torch.tensor(W_COLOUR, dtype=torch.float64)

    def grads(loss):
        gs = torch.autograd.grad(loss, wrt, retain_graph=True, allow_unused=True)      # (the depth output does not depend on sh)
        gs = [torch.zeros_like(t) if g_ is None else g_ for g_, t in zip(gs, wrt)]
        d = {k: g_.detach() for k, g_ in zip(keys, gs)}
        # means2D gradient as the published backward defines it: dL / d(NDC mean) = dL / d(pixel mean) * (W/2, H/2)
        d["m2"] = torch.stack([gs[-2].detach() * 0.5 * sc["W"], gs[-1].detach() * 0.5 * sc["H"]], 1)
        return d

    col, dep = [], []
    for y in range(sc["H"]):
        for x in range(sc["W"]):
            col.append(grads((oc[:, y, x] * wc).sum()))
            dep.append(grads(W_DEPTH * od[0, y, x]))
    stack = lambda lst: {k: torch.stack([d[k] for d in lst]) for k in GROUPS}
    return aux, stack(col), stack(dep)


@pytest.fixture(scope="module")
def refs():
    out = {}
    for name in SCENES:
        sc = build_scene(name)
        out[name] = (sc,) + oracle_reference(sc)
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_every_gaussian_is_blended_on_every_pixel(name, refs):
    sc, aux, _, _ = refs[name]
    H, W = sc["H"], sc["W"]
    pre = aux["pre"]
    px, py, conic, op = (pre[k].detach().numpy() for k in ("px", "py", "conic", "opacity"))
    ys, xs = np.mgrid[0:H, 0:W]
    dx, dy = px[:, None] - xs.reshape(-1)[None], py[:, None] - ys.reshape(-1)[None]
    power = -0.5 * (conic[:, 0, None] * dx * dx + conic[:, 2, None] * dy * dy) - conic[:, 1, None] * dx * dy
    alpha = op[:, None] * np.exp(power)
    print(name, "alpha range", alpha.min(), alpha.max(), "|cxy| min", np.abs(conic[:, 1]).min())
    assert power.max() <= 0 and alpha.min() >= 1.0 / 255.0 and alpha.max() < 0.99     # taken everywhere, never clamped
    assert (aux["n_contrib"] == N).all()                                              # ... and no pixel saturates before the last
    assert int(aux["ranges"][0, 1] - aux["ranges"][0, 0]) == N and len(aux["ranges"]) == 1
    assert np.abs(conic[:, 1]).min() > 1e-4 * np.abs(conic[:, [0, 2]]).max()
    assert len(set(np.round(pre["depth"].detach().numpy(), 6))) == N and 0.3 <= op.min() and op.max() <= 0.9
    assert (H % 16 == 0) == (name == "tile16x16") and (H % 16 == 0 or H % 16 > 8)    # rows13: a partial LOWER half-tile


def hip_one_hot_grads(sc, dev, with_depth):
    """One HIP forward, then one backward pass per pixel -> {group: [P, ...]} float64 CPU."""
    from syn3r_amd.raster import GaussianRasterizationSettings, rasterize_backward, rasterize_forward
    H, W = sc["H"], sc["W"]
    f = lambda t: t.to(dev, torch.float32).contiguous()
    st_ = GaussianRasterizationSettings(H, W, sc["tfx"], sc["tfy"], f(sc["bg"]), 1.0, f(sc["view"]), f(sc["proj"]), 3,
                                        f(sc["campos"]), False, False)
    _, _, _, _, st = rasterize_forward(f(sc["m"]), f(sc["sh"]), f(sc["o"]), f(sc["s"]), f(sc["q"]), None, st_)
    wc = torch.tensor(W_COLOUR, device=dev)
    out = {k: [] for k in GROUPS + ("m2z",)}
    for y in range(H):
        for x in range(W):
            gc = torch.zeros(3, H, W, device=dev)
            gc[:, y, x] = wc
            gd = None
            if with_depth:
                gd = torch.zeros(1, H, W, device=dev)
                gd[0, y, x] = W_DEPTH
            d_m3, d_m2, d_sh, d_op, d_sc, d_ro, _ = rasterize_backward(st, gc, gd, None)
            for k, t in zip(out, (d_m3, d_sc, d_ro, d_op, d_sh, d_m2[:, :2], d_m2[:, 2])):
                out[k].append(t)
    assert (torch.stack(out.pop("m2z")) == 0).all()
    return {k: torch.stack(v).cpu().double() for k, v in out.items()}


@pytest.mark.parametrize("with_depth", [False, True], ids=["colour", "colour+depth"])
@pytest.mark.parametrize("name", list(SCENES))
def test_one_hot_gradients_match_float64_autograd(name, with_depth, refs, gpu):
    sc, aux, col, dep = refs[name]
    got = hip_one_hot_grads(sc, gpu, with_depth)
    P = sc["H"] * sc["W"]
    worst = {}
    bad = []
    for k in GROUPS:
        ref = col[k] + dep[k] if with_depth else col[k]
        assert got[k].shape == ref.shape and ref.shape[0] == P
        diff = (got[k] - ref).reshape(P, -1).abs().max(1)[0]
        scale = ref.reshape(P, -1).abs().max(1)[0]
        assert float(scale.min()) > 0                       # every pass has a gradient in every group
        rel = diff / scale
        worst[k] = float(rel.max())
        for i in torch.nonzero(rel >= BAR).reshape(-1).tolist():
            bad.append((k, divmod(i, sc["W"]), float(rel[i])))
    print(name, "depth" if with_depth else "colour", {k: f"{v:.2e}" for k, v in worst.items()})
    assert not bad, (name, with_depth, len(bad), bad[:12])
