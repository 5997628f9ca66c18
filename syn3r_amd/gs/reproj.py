"""Host side of the trainer's multi-view photometric reprojection term (`OptimizationParams.reproj_weight`; csrc/reproj.hip,
`train_ops.photo_reprojection_loss`): the relative view of a (target, source) camera pair, the rule that picks a target's source
views, and the per-target cache of both.  Float64 numpy throughout; needs no GPU.

Pixel convention of the rasteriser (`ndc2pix`, csrc/raster_fwd.hip): pixel index x sits at fx X/Z + (W-1)/2 with fx = W / (2 tan(FoVx/2))
- NOT the W/2 of `Camera.get_calib_matrix_nerf`."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

MAX_SOURCES = 4                 # kRpMaxSources of csrc/reproj.hip
CAMERA_KINDS = ("train", "pseudo", "all")


class ReprojViews(NamedTuple):
    """What the kernel's tables are filled from, as fp32: `target_k` [4] = fx, fy, cx, cy of the target, `table` [S,16] = per source
    M (3 x 3, row-major), t, fx, fy, cx, cy with [M | t] = w2c_source c2w_target."""
    target_k: np.ndarray
    table: np.ndarray


def intrinsics(cam) -> np.ndarray:
    """(fx, fy, cx, cy) of a camera in the rasteriser's pixel convention, float64"""
    W, H = int(cam.image_width), int(cam.image_height)
    return np.array([W / (2.0 * math.tan(float(cam.FoVx) * 0.5)), H / (2.0 * math.tan(float(cam.FoVy) * 0.5)), (W - 1) * 0.5, (H - 1) * 0.5],
                    dtype=np.float64)


def _w2c(cam) -> np.ndarray:
    """the camera's CURRENT world-to-camera matrix from R (camera-to-world rotation) and T (world-to-camera translation), float64"""
    m = np.eye(4, dtype=np.float64)
    m[:3, :3] = np.asarray(cam.R, np.float64).T
    m[:3, 3] = np.asarray(cam.T, np.float64).reshape(3)
    return m


def relative_view(target, source) -> np.ndarray:
    """The 16 floats of a source for a target, float64: M (9), t (3), fx_s, fy_s, cx_s, cy_s; [M | t] = w2c_source inverse(w2c_target),
    from the cameras' current R, T, FoV."""
    rel = _w2c(source) @ np.linalg.inv(_w2c(target))
    return np.concatenate([rel[:3, :3].reshape(9), rel[:3, 3], intrinsics(source)])


def _centre(cam) -> np.ndarray:
    return -(np.asarray(cam.R, np.float64) @ np.asarray(cam.T, np.float64).reshape(3))


def select_sources(target, cameras: Sequence, count: int, max_angle: float) -> List:
    """The source rule (this project's choice: UNPINNED): of `cameras` (the input views), excluding `target` itself, those that have
    an image of the target's H, W and a viewing direction within `max_angle` degrees of the target's; the `count` nearest by
    camera-centre distance, ties in list order.  May be empty: the target then skips the term."""
    hw = (int(target.image_height), int(target.image_width))
    d_t, c_t = np.asarray(target.R, np.float64)[:, 2], _centre(target)
    found = []
    for k, cam in enumerate(cameras):
        if cam is target or getattr(cam, "original_image", None) is None:
            continue
        if (int(cam.image_height), int(cam.image_width)) != hw or tuple(cam.original_image.shape) != (3,) + hw:
            continue
        d = np.asarray(cam.R, np.float64)[:, 2]
        cosang = float(d @ d_t) / (float(np.linalg.norm(d)) * float(np.linalg.norm(d_t)) + 1e-300)
        if math.degrees(math.acos(min(1.0, max(-1.0, cosang)))) > max_angle:
            continue
        found.append((float(np.linalg.norm(_centre(cam) - c_t)), k, cam))
    found.sort(key=lambda f: (f[0], f[1]))
    return [f[2] for f in found[:max(int(count), 0)]]


def check_options(opt) -> None:
    """ValueError for option values the term cannot run with"""
    if opt.reproj_cameras not in CAMERA_KINDS:
        raise ValueError(f"OptimizationParams.reproj_cameras must be 'train', 'pseudo' or 'all', got {opt.reproj_cameras!r}")
    if not (math.isfinite(float(opt.reproj_weight)) and float(opt.reproj_weight) >= 0.0):
        raise ValueError(f"OptimizationParams.reproj_weight must be finite and >= 0, got {opt.reproj_weight!r}")
    if not 1 <= int(opt.reproj_sources) <= MAX_SOURCES:
        raise ValueError(f"OptimizationParams.reproj_sources must be in [1, {MAX_SOURCES}], got {opt.reproj_sources!r}")
    if not 0.0 < float(opt.reproj_alpha_min) <= 1.0:
        raise ValueError(f"OptimizationParams.reproj_alpha_min must be in (0, 1], got {opt.reproj_alpha_min!r}")
    if not 0.0 < float(opt.reproj_max_angle) <= 180.0:
        raise ValueError(f"OptimizationParams.reproj_max_angle must be in (0, 180] degrees, got {opt.reproj_max_angle!r}")
    if int(opt.reproj_from_iter) < 0:
        raise ValueError(f"OptimizationParams.reproj_from_iter must be >= 0, got {opt.reproj_from_iter!r}")


class ReprojCache:
    """Per target camera: its source cameras, their images and the fp32 tables.  An entry is keyed by the IDENTITY of the
    `world_view_transform` tensors of the target and of every candidate camera (`Camera.set_pose` makes new tensors, so a pose moved
    by `pose_opt` rebuilds it), by the candidate list (its cameras, in order) and by the two options of the rule.  `builds` counts
    rebuilds.  An entry holds its cameras and their images alive: `retain` drops those of cameras that left the scene
    (`GSTrainer.update_cameras` calls it).  Nothing of it goes into checkpoints."""

    def __init__(self):
        self._entries = {}
        self.builds = 0

    def get(self, target, cameras: Sequence, count: int, max_angle: float):
        """-> (source images, ReprojViews, source cameras), or None for a target without a source"""
        key = (int(count), float(max_angle))
        e = self._entries.get(id(target))
        if e is not None and e[0] is target and e[1] is target.world_view_transform and e[2] == key and len(e[3]) == len(cameras) \
                and all(c is cam and w is cam.world_view_transform and im is cam.original_image for (c, w, im), cam in zip(e[3], cameras)):
            return e[4]
        sources = select_sources(target, cameras, count, max_angle)
        result = None
        if sources:
            table = np.stack([relative_view(target, s) for s in sources]).astype(np.float32)
            result = ([s.original_image for s in sources], ReprojViews(intrinsics(target).astype(np.float32), table), sources)
        self._entries[id(target)] = (target, target.world_view_transform, key,
                                     [(c, c.world_view_transform, c.original_image) for c in cameras], result)
        self.builds += 1
        return result

    def clear(self) -> None:
        self._entries.clear()

    def retain(self, cameras: Sequence) -> None:
        """Drop the entries whose target is not one of `cameras` (an entry holds its target, the candidates and their images alive)"""
        keep = {id(c) for c in cameras}
        self._entries = {k: e for k, e in self._entries.items() if k in keep and any(e[0] is c for c in cameras)}


def eligible(opt, cam, iteration: int) -> bool:
    """Whether a step on `cam` at `iteration` carries the term, before the source rule is asked"""
    if not float(opt.reproj_weight) > 0.0 or iteration < int(opt.reproj_from_iter):
        return False
    if opt.reproj_cameras not in CAMERA_KINDS:
        raise ValueError(f"OptimizationParams.reproj_cameras must be 'train', 'pseudo' or 'all', got {opt.reproj_cameras!r}")
    pseudo = bool(getattr(cam, "is_pseudo", False))
    if (opt.reproj_cameras == "train" and pseudo) or (opt.reproj_cameras == "pseudo" and not pseudo):
        return False
    return getattr(cam, "original_image", None) is not None


def sources_for(cache: ReprojCache, opt, cam, cameras: Sequence, iteration: int) -> Optional[tuple]:
    """`ReprojCache.get` for a step on `cam` when the term acts on it, else None"""
    if not eligible(opt, cam, iteration):
        return None
    check_options(opt)
    return cache.get(cam, cameras, int(opt.reproj_sources), float(opt.reproj_max_angle))
