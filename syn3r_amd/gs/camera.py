"""The cameras of the trainer (`gs/trainer.py`) and the registry the orchestrator touches.  Camera conventions follow the published
3DGS/FSGS code: `world_view_transform` and `full_proj_transform` are the TRANSPOSED matrices."""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np
import torch


def _world2view(R: np.ndarray, t: np.ndarray) -> np.ndarray:
    Rt = np.zeros((4, 4), dtype=np.float32)
    Rt[:3, :3] = R.transpose()
    Rt[:3, 3] = t
    Rt[3, 3] = 1.0
    return Rt


def _projection(znear: float, zfar: float, fovx: float, fovy: float) -> torch.Tensor:
    ty, tx = math.tan(fovy / 2), math.tan(fovx / 2)
    top, right = ty * znear, tx * znear
    P = torch.zeros(4, 4)
    P[0, 0] = znear / right
    P[1, 1] = znear / top
    P[3, 2] = 1.0
    P[2, 2] = zfar / (zfar - znear)
    P[2, 3] = -(zfar * znear) / (zfar - znear)
    return P


class Camera:
    """`FSGS.scene.cameras.Camera(colmap_id, R, T, FoVx, FoVy, image, gt_alpha_mask, image_name, uid, trans, scale,
    data_device, cam_confidence)` as constructed at diffusionGS.py:161-163.  R is camera-to-world rotation and T the
    world-to-camera translation (COLMAP/3DGS convention).  `depth_image`: the monocular depth prior [H,W] (or [1,H,W]) of the
    view, named as in FSGS' camera; the trainer's depth-correlation term reads it (None: `GSTrainer.depth_net` fills it in, or
    the view has no prior).
    `confidence_map` (EXTENSION, not in the reference's camera; default None): a per-pixel weight [H,W] (or [1,H,W]) in [0,1] for
    the photometric loss of this view (`train_ops.photometric_loss(weight_map=)`), on top of the scalar `cam_confidence`; stored as
    fp32 [H,W] on `data_device`, its shape checked against the image's.  Also settable as an attribute.  `gt_alpha_mask` stays
    ignored: in published 3DGS it multiplies the image, which is a different thing.
    `depth_edge_weights` (EXTENSION; default None): the caller's own edge weights [2,H,W] = [wx, wy] for the trainer's depth-smoothness
    term (`OptimizationParams.depth_smooth_weight`), stored as fp32 on `data_device` and then NEVER recomputed; None: the trainer
    computes them from `original_image` once (`GSTrainer.depth_edge_weights`) and keeps them in `_depth_edge_cache`, 8 bytes per
    pixel, with the gamma and the image they were made from.  Also settable as an attribute."""

    def __init__(self, colmap_id, R, T, FoVx, FoVy, image, gt_alpha_mask=None, image_name="", uid=0,
                 trans=np.array([0.0, 0.0, 0.0]), scale=1.0, data_device="cuda", cam_confidence: float = 1.0, depth_image=None,
                 confidence_map=None, depth_edge_weights=None):
        self.uid, self.colmap_id, self.image_name = uid, colmap_id, image_name
        self.R, self.T, self.FoVx, self.FoVy = np.asarray(R, np.float32), np.asarray(T, np.float32), FoVx, FoVy
        self.cam_confidence = float(cam_confidence)
        self.is_pseudo = False           # set by GSTrainer.update_cameras for SVD pseudo-views
        self.data_device = torch.device(data_device)
        self.original_image = None
        self.image_height = self.image_width = None      # without an image: `from_w2c` sets the size
        if image is not None:
            self.original_image = torch.as_tensor(image, dtype=torch.float32).clamp(0.0, 1.0).to(self.data_device)
            self.image_height, self.image_width = self.original_image.shape[1:]
        self.zfar, self.znear = 100.0, 0.01
        w2c = torch.tensor(_world2view(self.R, self.T))
        self.world_view_transform = w2c.transpose(0, 1).to(self.data_device)
        self.projection_matrix = _projection(self.znear, self.zfar, FoVx, FoVy).transpose(0, 1).to(self.data_device)
        self.full_proj_transform = self.world_view_transform @ self.projection_matrix
        self.camera_center = self.world_view_transform.inverse()[3, :3]
        self.depth_image = None
        if depth_image is not None:
            d = torch.as_tensor(depth_image, dtype=torch.float32).to(self.data_device)
            self.depth_image = (d[0] if d.dim() == 3 and d.shape[0] == 1 else d).contiguous()
        self._confidence_map = None
        self.confidence_map = confidence_map
        self._depth_edge_weights = None
        self._depth_edge_cache = None    # (gamma, image, image version, weights) of GSTrainer.depth_edge_weights
        self.depth_edge_weights = depth_edge_weights

    @property
    def confidence_map(self) -> Optional[torch.Tensor]:
        return self._confidence_map

    @confidence_map.setter
    def confidence_map(self, m):
        if m is None:
            self._confidence_map = None
            return
        m = torch.as_tensor(m).detach().to(dtype=torch.float32, device=self.data_device)
        m = m[0] if m.dim() == 3 and m.shape[0] == 1 else m
        hw = (self.image_height, self.image_width)
        if hw[0] is None:
            raise ValueError("Camera: a confidence_map needs a camera with an image size")
        if m.dim() != 2 or tuple(m.shape) != (int(hw[0]), int(hw[1])):
            raise ValueError(f"Camera: confidence_map must be [H,W] or [1,H,W] for the image's H, W = ({int(hw[0])}, {int(hw[1])}); "
                             f"got {tuple(m.shape)}")
        self._confidence_map = m.contiguous()

    @property
    def depth_edge_weights(self) -> Optional[torch.Tensor]:
        return self._depth_edge_weights

    @depth_edge_weights.setter
    def depth_edge_weights(self, w):
        if w is None:
            self._depth_edge_weights = None
            return
        w = torch.as_tensor(w).detach().to(dtype=torch.float32, device=self.data_device)
        hw = (self.image_height, self.image_width)
        if hw[0] is None:
            raise ValueError("Camera: depth_edge_weights need a camera with an image size")
        if tuple(w.shape) != (2, int(hw[0]), int(hw[1])):
            raise ValueError(f"Camera: depth_edge_weights must be [2,H,W] for the image's H, W = ({int(hw[0])}, {int(hw[1])}); "
                             f"got {tuple(w.shape)}")
        self._depth_edge_weights = w.contiguous()

    @classmethod
    def from_w2c(cls, w2c: np.ndarray, K: np.ndarray, H: int, W: int, image=None, **kw):
        """Build from a 4x4 world-to-camera matrix and intrinsics (the orchestrator's pose format)."""
        fovx = 2 * math.atan(W / (2 * K[0, 0]))
        fovy = 2 * math.atan(H / (2 * K[1, 1]))
        cmap, edge = kw.pop("confidence_map", None), kw.pop("depth_edge_weights", None)
        cam = cls(0, np.asarray(w2c[:3, :3]).T, np.asarray(w2c[:3, 3]), fovx, fovy, image, **kw)
        if image is None:
            cam.image_height, cam.image_width = H, W
        cam.confidence_map = cmap                      # (after the size is known)
        cam.depth_edge_weights = edge
        return cam

    def set_pose(self, R, T):
        """Move the camera (EXTENSION: pose refinement, `GSTrainer.apply_pose_updates`): `R` camera-to-world rotation, `T`
        world-to-camera translation, as the constructor takes them.  `world_view_transform`, `full_proj_transform` and
        `camera_center` (= -R_w2c^T T) are rebuilt as NEW tensors: the rasteriser's host copies of them are keyed by tensor identity
        and version, so a moved camera can never be rendered from a stale matrix.  The projection does not change."""
        self.R, self.T = np.asarray(R, np.float32).copy(), np.asarray(T, np.float32).reshape(3).copy()
        w2c = torch.tensor(_world2view(self.R, self.T))
        self.world_view_transform = w2c.transpose(0, 1).to(self.data_device)
        self.full_proj_transform = self.world_view_transform @ self.projection_matrix
        centre = -(self.R.astype(np.float64) @ self.T.astype(np.float64))
        self.camera_center = torch.tensor(centre, dtype=torch.float32).to(self.data_device)

    def get_image(self):
        return self.original_image

    def get_calib_matrix_nerf(self):
        """(K, w2c) as diffusionGS.py:67-70 reads them."""
        fx = self.image_width / (2 * math.tan(self.FoVx / 2))
        fy = self.image_height / (2 * math.tan(self.FoVy / 2))
        K = torch.tensor([[fx, 0, self.image_width / 2], [0, fy, self.image_height / 2], [0, 0, 1]], dtype=torch.float32)
        return K, self.world_view_transform.transpose(0, 1).cpu()



class _Scene:
    """The part of FSGS' `Scene` the orchestrator touches: `model_path` (checkpoint directory, diffusionGS.py:1611),
    `train_cameras` ({resolution scale: [Camera]}; backed up and restored around a finetune, :1627,1641) and
    `getTrainCameras()`.  Pseudo-views appended by `update_cameras` carry `is_pseudo`; `getTrainCameras` returns the
    real input views, `getPseudoCameras` the appended ones."""

    def __init__(self, cams, model_path: Optional[str] = None):
        self.train_cameras: Dict[float, List[Camera]] = {1.0: list(cams)}
        self.model_path = model_path

    def getTrainCameras(self, scale: float = 1.0, ordered: bool = False):
        return [c for c in self.train_cameras[scale] if not getattr(c, "is_pseudo", False)]

    def getPseudoCameras(self, scale: float = 1.0):
        return [c for c in self.train_cameras[scale] if getattr(c, "is_pseudo", False)]
