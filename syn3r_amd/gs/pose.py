"""Camera-pose refinement, host side (EXTENSION: the reference has no pose refinement, nothing reference-held pins any of this).

The rasteriser returns the gradient of the loss with respect to its three camera inputs taken as INDEPENDENT
(`rasterize_backward(camera_grad_out=)`, syn3r_raster_backward_cam: view[16], proj[16], campos[3] in storage order).  This module
turns those 35 numbers into the gradient of a 6-vector on the pose and applies an Adam step to it.  The maths is float64 numpy: a
few dozen flops per camera and update.  `PoseTable` is what the trainer holds: the device table the rasteriser sums into.

Convention: world-to-camera M = [R | t] (4 x 4, bottom row 0 0 0 1), twist xi = (rho, phi) with the TRANSLATION FIRST, LEFT
perturbation M' = Exp(xi) M.  A `Camera` stores R as camera-to-world (R_c2w = R^T) and T = t, the published 3DGS convention.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .. import _lib as L

_SMALL = 1e-4        # below it the series of the three coefficients (relative error ~ theta^4 / 20160 and smaller: < 1e-20)


def hat(w: np.ndarray) -> np.ndarray:
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]], dtype=np.float64)


def se3_exp(xi) -> np.ndarray:
    """Exp of the twist xi = (rho, phi) as a 4 x 4 matrix: R = I + A K + B K^2 (Rodrigues), t = (I + B K + C K^2) rho with K = hat(phi),
    theta = |phi|, A = sin(theta) / theta, B = (1 - cos(theta)) / theta^2, C = (theta - sin(theta)) / theta^3; their series for small
    theta."""
    xi = np.asarray(xi, dtype=np.float64).reshape(6)
    rho, phi = xi[:3], xi[3:]
    th2 = float(phi @ phi)
    th = np.sqrt(th2)
    if th < _SMALL:
        A = 1.0 - th2 / 6.0 + th2 * th2 / 120.0
        B = 0.5 - th2 / 24.0 + th2 * th2 / 720.0
        Cc = 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0
    else:
        A = np.sin(th) / th
        B = (1.0 - np.cos(th)) / th2
        Cc = (th - np.sin(th)) / (th2 * th)
    K = hat(phi)
    K2 = K @ K
    out = np.eye(4, dtype=np.float64)
    out[:3, :3] = np.eye(3) + A * K + B * K2
    out[:3, 3] = (np.eye(3) + B * K + Cc * K2) @ rho
    return out


def camera_w2c(cam) -> np.ndarray:
    """The 4 x 4 world-to-camera matrix of a `Camera` (R is camera-to-world, T the world-to-camera translation), float64."""
    M = np.eye(4, dtype=np.float64)
    M[:3, :3] = np.asarray(cam.R, dtype=np.float64).T
    M[:3, 3] = np.asarray(cam.T, dtype=np.float64)
    return M


def tangent_from_raw(raw35, cam=None, *, w2c: Optional[np.ndarray] = None, projection: Optional[np.ndarray] = None) -> np.ndarray:
    """d loss / d xi at xi = 0 of M' = Exp(xi) M, from the rasteriser's raw camera gradient.

    `raw35`: dV = d loss / d world_view_transform [4,4], dF = d loss / d full_proj_transform [4,4] (both TRANSPOSED storage, as the
    camera holds them: world_view_transform = M^T, full_proj_transform = world_view_transform @ projection_matrix = (P M)^T) and
    dc = d loss / d camera_center [3].  `cam`: a `Camera` (its R, T and `projection_matrix` are read), or give `w2c` (4 x 4) and
    `projection` (P, 4 x 4, NOT transposed) directly.

    With the three tied to the pose: d loss / dM = G = dV^T + P^T dF^T, top 3 x 4 = [G_R | g_t]; the centre c = -R^T t moves as
    c' = c - R^T rho (its rotation terms cancel to first order).  Hence
        d loss / d rho = g_t - R dc          d loss / d phi = sum_{j = 0..3} M[:3, j] x G[:3, j]."""
    raw = np.asarray(raw35, dtype=np.float64).reshape(35)
    if cam is not None:
        w2c = camera_w2c(cam)
        projection = np.asarray(cam.projection_matrix.detach().cpu().numpy(), dtype=np.float64).T
    M, P = np.asarray(w2c, dtype=np.float64), np.asarray(projection, dtype=np.float64)
    dV, dF, dc = raw[:16].reshape(4, 4), raw[16:32].reshape(4, 4), raw[32:]
    G = dV.T + P.T @ dF.T
    R = M[:3, :3]
    d_rho = G[:3, 3] - R @ dc
    d_phi = np.zeros(3)
    for j in range(4):
        d_phi += np.cross(M[:3, j], G[:3, j])
    return np.concatenate([d_rho, d_phi])


class PoseOptimizer:
    """Adam on the 6-vector of a camera pose (bias-corrected, betas 0.9 / 0.999, eps 1e-15 as the Gaussians' optimiser; torch.optim.Adam's
    arithmetic), one rate for the translation part rho and one (radians) for the rotation part phi.  The state of a camera is a dict
    {"m": [6], "v": [6], "t": int}; `GSTrainer` keeps it on the camera object.  The rates are CHOSEN, not taken from any source:
    UNPINNED and scene dependent."""

    def __init__(self, lr_rotation: float = 1e-3, lr_translation: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-15):
        self.lr_rotation, self.lr_translation = float(lr_rotation), float(lr_translation)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)

    @staticmethod
    def new_state() -> dict:
        return {"m": np.zeros(6), "v": np.zeros(6), "t": 0}

    def step_vector(self, state: dict, grad) -> np.ndarray:
        """Advance `state` by one gradient and return the step (what Adam subtracts from its parameter)."""
        g = np.asarray(grad, dtype=np.float64).reshape(6)
        b1, b2 = self.betas
        state["t"] = int(state["t"]) + 1
        state["m"] = b1 * state["m"] + (1.0 - b1) * g
        state["v"] = b2 * state["v"] + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** state["t"], 1.0 - b2 ** state["t"]
        lr = np.array([self.lr_translation] * 3 + [self.lr_rotation] * 3)
        denom = np.sqrt(state["v"]) / np.sqrt(bc2) + self.eps
        return (lr / bc1) * state["m"] / denom

    def update(self, w2c: np.ndarray, state: dict, grad) -> np.ndarray:
        """M <- Exp(-step) M, the rotation brought back onto SO(3) by an SVD (U V^T; a pose never reflects: det stays +1)."""
        M = se3_exp(-self.step_vector(state, grad)) @ np.asarray(w2c, dtype=np.float64)
        U, _, Vt = np.linalg.svd(M[:3, :3])
        R = U @ Vt
        if np.linalg.det(R) < 0.0:
            U[:, -1] = -U[:, -1]
            R = U @ Vt
        out = np.eye(4, dtype=np.float64)
        out[:3, :3], out[:3, 3] = R, M[:3, 3]
        return out


class PoseTable:
    """The trainer's side of `OptimizationParams.pose_opt`: the device table [C,35] of summed camera gradients, one row per registered
    camera, the cameras of its rows (the list object and its members as they were when it was made) and the host count of steps per
    row.  It reads the trainer's `opt`, `scene`, `iteration`, `gaussians` (for the device) and `spatial_lr_scale` when it needs them,
    and tells the trainer's 3D-filter cache (`filter3d.invalidate_cameras`) when cameras have moved."""

    def __init__(self, trainer):
        self.trainer = trainer
        self.updates = 0                  # camera moves applied so far (`apply`)
        self.drop()

    def drop(self):
        """No table (the state with the option off); `sync` makes a fresh one at the next step that wants a camera gradient."""
        self.table, self.list, self.cams, self.counts = None, None, [], []

    def sync(self):
        """Keep the gradient table in step with `scene.train_cameras[1.0]`: when the list is another object or has another length
        (`update_cameras`, the orchestrator's restore) what is pending is applied to the cameras of the old rows and a fresh table is
        made.  The Adam state lives on the camera objects, so it survives."""
        cams = self.trainer.scene.train_cameras[1.0]
        if self.table is not None and self.list is cams and len(self.cams) == len(cams):
            return
        if self.table is not None:
            self.apply()
        dev = self.trainer.gaussians._xyz.device
        self.list, self.cams, self.counts = cams, list(cams), [0] * len(cams)
        self.table = torch.zeros((max(len(cams), 1), L.CAMERA_GRAD), dtype=torch.float32, device=dev)

    def row(self, cam) -> Optional[int]:
        """The table row of `cam` if this step's camera gradient is wanted, else None: the option on and started, the camera registered,
        of the chosen kind, and not the first training camera (the gauge: without a fixed camera the world frame drifts)."""
        o = self.trainer.opt
        if not o.pose_opt or self.trainer.iteration < int(o.pose_opt_from_iter):
            return None
        self.sync()
        row = next((i for i, c in enumerate(self.cams) if c is cam), None)
        if row is None:
            return None
        pseudo = bool(getattr(cam, "is_pseudo", False))
        if (pseudo and o.pose_opt_cameras == "train") or (not pseudo and o.pose_opt_cameras == "pseudo"):
            return None
        train = self.trainer.scene.getTrainCameras()
        if train and train[0] is cam:
            return None
        return row

    def count(self, row: Optional[int]):
        """One more step's camera gradient has been ADDED to `row` (None: this step wanted none)."""
        if row is not None:
            self.counts[row] += 1

    def apply(self) -> int:
        """ONE host read of the table; every camera with a non-zero count: mean raw gradient -> `tangent_from_raw` -> one Adam step
        (`PoseOptimizer`, state on the camera object) -> `Camera.set_pose`.  Then the table and the counts restart and the 3D
        filter's camera table is dropped (`ensure_filter_3D` rebuilds it from the moved poses).  Returns the number of cameras moved.
        Independent of the density control: the camera gradient belongs to the camera, whatever happened to the Gaussians."""
        if self.table is None or not any(self.counts):
            return 0
        host = self.table.detach().cpu().double().numpy()
        o = self.trainer.opt
        popt, moved = PoseOptimizer(lr_rotation=float(o.pose_lr_rotation),
                                    lr_translation=float(o.pose_lr_translation) * float(self.trainer.spatial_lr_scale)), 0
        for row, (cam, n) in enumerate(zip(self.cams, self.counts)):
            if n == 0:
                continue
            grad = tangent_from_raw(host[row] / float(n), cam)
            if not np.all(np.isfinite(grad)):
                continue                                   # (a degenerate render: leave the camera where it is)
            state = getattr(cam, "pose_adam", None)
            if state is None:
                state = cam.pose_adam = popt.new_state()
            M = popt.update(camera_w2c(cam), state, grad)
            cam.set_pose(M[:3, :3].T, M[:3, 3])
            moved += 1
        self.table.zero_()
        self.counts = [0] * len(self.counts)
        self.trainer.filter3d.invalidate_cameras()
        self.updates += moved
        return moved

    def flush(self) -> int:
        """Apply what is pending and start a fresh table at the next step (`update_cameras`, `reset_gs`, the orchestrator's restore of
        the camera list).  Nothing with the option off."""
        if self.table is None:
            return 0
        moved = self.apply()
        self.drop()
        return moved

    def capture(self) -> list:
        """Per registered camera: index, kind, R, T and the Adam state, as tensors (the checkpoint loader reads tensors only)."""
        out = []
        for i, cam in enumerate(self.trainer.scene.train_cameras[1.0]):
            st = getattr(cam, "pose_adam", None)
            e = {"index": i, "is_pseudo": int(bool(getattr(cam, "is_pseudo", False))), "R": torch.from_numpy(np.array(cam.R, np.float32)),
                 "T": torch.from_numpy(np.array(cam.T, np.float32))}
            if st is not None:
                e.update(m=torch.from_numpy(np.array(st["m"], np.float64)), v=torch.from_numpy(np.array(st["v"], np.float64)), t=int(st["t"]))
            out.append(e)
        return out

    def restore(self, entries: list):
        """Entry i goes to registered camera i when there is one of the same kind (a checkpoint written with pseudo-views registered
        may be loaded after the list was restored: their entries are skipped)."""
        cams = self.trainer.scene.train_cameras[1.0]
        for e in entries:
            i = int(e["index"])
            if i >= len(cams) or int(bool(getattr(cams[i], "is_pseudo", False))) != int(e["is_pseudo"]):
                continue
            cams[i].set_pose(e["R"].cpu().numpy(), e["T"].cpu().numpy())
            if "m" in e:
                cams[i].pose_adam = {"m": e["m"].cpu().double().numpy().copy(), "v": e["v"].cpu().double().numpy().copy(), "t": int(e["t"])}
            elif hasattr(cams[i], "pose_adam"):
                del cams[i].pose_adam
        self.drop()                                    # gradients summed at the poses just replaced are dropped, not applied
        self.trainer.filter3d.invalidate_cameras()
