"""float64 reference of the rasteriser's camera gradient (syn3r_raster_backward_cam, `rasterize_backward(camera_grad_out=)`), built
from oracle/raster_oracle.py, tests/raster_aa_ref.py and tests/raster_f3d_ref.py WITHOUT touching them and never from the code under
test: `RO.preprocess` is differentiable torch in `viewmatrix`, `projmatrix` and `campos`, so the three are made float64 LEAF tensors,
the scene is rendered with them, and `.backward()` of sum(wc colour) + sum(wd depth) + sum(wa alpha) (raster_aa_ref.loss_weights)
leaves the three gradients - each in its tensor's storage order, the three taken as independent inputs: the layout of the entry.

The scenes' own camera is the identity, which would hide any mistake in the rotation part W of the view matrix: every reference here
uses w2c = Exp(XI0) with look_at_camera's projection, view = w2c^T, full = (P w2c)^T, campos = -R^T t.  Exp is
torch.linalg.matrix_exp of the 4 x 4 twist (translation first), not syn3r_amd.gs.pose.se3_exp.

References are computed once per case and cached; callers must not modify them."""
import numpy as np
import torch

import raster_aa_ref as A
import raster_f3d_ref as F
from oracle import raster_oracle as RO

XI0 = (0.10, -0.05, 0.20, 0.08, -0.12, 0.05)
MODES = ("plain", "antialias", "filter3d", "filter3d+antialias")


def twist(xi):
    """The 4 x 4 matrix of the twist xi = (rho, phi): [[hat(phi), rho], [0, 0]]; differentiable in xi."""
    xi = torch.as_tensor(xi, dtype=torch.float64)
    z = torch.zeros((), dtype=torch.float64)
    r, p = xi[:3], xi[3:]
    return torch.stack([torch.stack([z, -p[2], p[1], r[0]]), torch.stack([p[2], z, -p[0], r[1]]),
                        torch.stack([-p[1], p[0], z, r[2]]), torch.stack([z, z, z, z])])


def exp_twist(xi):
    return torch.linalg.matrix_exp(twist(xi))


def projection(H, W):
    """look_at_camera's projection P (not transposed): with its identity pose the full transform is P^T."""
    _, full, _, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float64)
    return full.t().contiguous(), tfx, tfy


def camera_tensors(w2c, P):
    """(view, full, campos) in the transposed storage of the cameras, from a world-to-camera matrix; differentiable in w2c."""
    return w2c.t(), (P @ w2c).t(), -(w2c[:3, :3].t() @ w2c[:3, 3])


def with_camera(sc, xi=XI0):
    """A copy of a scene dict seen from w2c = Exp(xi): `view`, `proj`, `campos` replaced, `P` and `w2c` added."""
    P, tfx, tfy = projection(sc["H"], sc["W"])
    w2c = exp_twist(xi)
    view, full, campos = camera_tensors(w2c, P)
    out = dict(sc)
    out.update(view=view.contiguous(), proj=full.contiguous(), campos=campos.contiguous(), tfx=tfx, tfy=tfy, P=P, w2c=w2c)
    return out


def render(sc, deg, mode="plain"):
    """The float64 render of `sc` in one of MODES through the matching reference module -> (color, radii, depth, alpha, aux)."""
    aa = mode.endswith("antialias")
    if mode.startswith("filter3d"):
        return F.rasterize(sc, deg, sc["f"], aa)[0]
    return A.rasterize(sc, deg, aa)[0]


def loss_of(out, weights, depth_grad=True):
    wc, wd, wa = weights
    loss = (out[0] * wc).sum() + (out[3] * wa).sum()
    return loss + (out[2] * wd).sum() if depth_grad else loss


def camera_gradient(sc, deg, mode="plain", depth_grad=True, weights=None):
    """-> dict(raw [35] float64 = (d/dview [16], d/dproj [16], d/dcampos [3]) in storage order, valid [N] bool, weights, loss)."""
    weights = weights if weights is not None else A.loss_weights(sc["H"], sc["W"])
    leaves = {k: sc[k].detach().to(torch.float64).clone().requires_grad_(True) for k in ("view", "proj", "campos")}
    s2 = dict(sc)
    s2.update(leaves)
    out = render(s2, deg, mode)
    loss = loss_of(out, weights, depth_grad)
    loss.backward()
    g = lambda k: leaves[k].grad if leaves[k].grad is not None else torch.zeros_like(leaves[k])      # (degree 0: campos is unused)
    raw = torch.cat([g("view").reshape(-1), g("proj").reshape(-1), g("campos").reshape(-1)])
    return dict(raw=raw, valid=out[4]["pre"]["valid"], weights=weights, loss=float(loss.detach()))


_scenes, _cache = {}, {}


def scene(shape, mode="plain"):
    """raster_aa_ref's scene of `shape` (raster_f3d_ref's, with its filter "f", in the filtered modes) seen from Exp(XI0)."""
    key = (shape, mode.startswith("filter3d"))
    if key not in _scenes:
        N, H, W, conf, deg, scale = shape
        _scenes[key] = with_camera(F.scene(shape) if key[1] else A.scene(N, H, W, conf, scale))
    return _scenes[key]


def reference(shape, mode="plain", depth_grad=True):
    key = (shape, mode, bool(depth_grad))
    if key not in _cache:
        sc = scene(shape, mode)
        ref = camera_gradient(sc, shape[4], mode, depth_grad)
        ref.update(sc=sc, deg=shape[4])
        _cache[key] = ref
    return _cache[key]


def subset(sc, idx):
    """The scene with the Gaussians `idx` alone (a slice or an index tensor)."""
    out = dict(sc)
    for k in A.PARAMS:
        out[k] = sc[k][idx].clone()
    out["cf"] = sc["cf"][idx].clone() if sc["cf"] is not None else None
    if "f" in sc:
        out["f"] = sc["f"][idx].clone()
    out["N"] = int(out["m"].shape[0])
    return out


def tangent_by_autograd(sc, deg, mode="plain", depth_grad=True, weights=None):
    """d loss / d xi at xi = 0 of the same loss rendered from Exp(xi) w2c: autograd through the three tied camera tensors."""
    weights = weights if weights is not None else A.loss_weights(sc["H"], sc["W"])
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    view, full, campos = camera_tensors(exp_twist(xi) @ sc["w2c"], sc["P"])
    s2 = dict(sc)
    s2.update(view=view, proj=full, campos=campos)
    loss_of(render(s2, deg, mode), weights, depth_grad).backward()
    return xi.grad.clone()


def tangent_by_differences(sc, deg, h=1e-6, mode="plain", depth_grad=True, weights=None):
    """central differences of the full re-render; a check of the CONVENTION on a scene where no discontinuity of the rasteriser
    (1/255, power <= 0, tile rectangles) lies within h - never the kernel's checker."""
    weights = weights if weights is not None else A.loss_weights(sc["H"], sc["W"])
    out = np.zeros(6)
    with torch.no_grad():
        for k in range(6):
            val = []
            for sgn in (1.0, -1.0):
                xi = torch.zeros(6, dtype=torch.float64)
                xi[k] = sgn * h
                view, full, campos = camera_tensors(exp_twist(xi) @ sc["w2c"], sc["P"])
                s2 = dict(sc)
                s2.update(view=view.contiguous(), proj=full.contiguous(), campos=campos.contiguous())
                val.append(float(loss_of(render(s2, deg, mode), weights, depth_grad)))
            out[k] = (val[0] - val[1]) / (2.0 * h)
    return out
