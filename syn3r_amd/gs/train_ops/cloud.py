"""Point-cloud operators on the HIP library: the exact 3-nearest-neighbour search and FSGS' proximity-guided unpooling on its graph
(csrc/knn.hip), and Mip-Splatting's 3D smoothing filter with the camera table it reads (csrc/filter3d.hip)."""
from __future__ import annotations

import torch

from ... import _lib as L


def knn3_mean_dist2(points: torch.Tensor) -> torch.Tensor:
    """Mean squared distance of every point of a [n,3] fp32 cloud (n >= 4) to its three nearest neighbours:
    `distCUDA2` of the simple-knn extension, which FSGS' create_from_pcd turns into the initial Gaussian scales
    (model/diffusionGS.py:1685-1687 -> reset_gaussians_from_pcd).  Exact search on the device (csrc/knn.hip)."""
    L.require_gpu(points)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("knn3_mean_dist2: points must be a float32 [n,3] tensor")
    pts = points.detach().contiguous()
    n = pts.shape[0]
    lib = L.load()
    out = torch.empty(n, dtype=torch.float32, device=pts.device)
    ws = L.workspace(pts.device, lib.syn3r_knn3_workspace_bytes(n), "knn3")
    L.check(lib.syn3r_knn3_mean_dist2(L.ptr(pts), n, L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr(pts.device)), "knn3_mean_dist2")
    return out


def _cloud_arg(who: str, points: torch.Tensor) -> torch.Tensor:
    L.require_gpu(points)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError(f"{who}: points must be a float32 [n,3] tensor")
    return points.detach().contiguous()


def knn3_graph(points: torch.Tensor):
    """The directed 3-nearest-neighbour graph of a [n,3] fp32 cloud (n >= 4): (dist2 [n,3] fp32, index [n,3] int32), per point the
    three other points nearest first, ties broken by the smaller index (`syn3r_knn3_graph`, csrc/knn.hip: the search of
    `knn3_mean_dist2` keeping the indices; `((d0 + d1) + d2) / 3` equals that function's result bit for bit).  The proximity graph
    of FSGS' Gaussian unpooling (`proximity_unpool`)."""
    pts = _cloud_arg("knn3_graph", points)
    n = pts.shape[0]
    lib = L.load()
    dist2 = torch.empty((n, 3), dtype=torch.float32, device=pts.device)
    index = torch.empty((n, 3), dtype=torch.int32, device=pts.device)
    ws = L.workspace(pts.device, lib.syn3r_knn3_graph_workspace_bytes(n), "knn3")
    L.check(lib.syn3r_knn3_graph(L.ptr(pts), n, L.ptr(dist2), L.ptr(index), L.ptr(ws), ws.numel(), L.stream_ptr(pts.device)), "knn3_graph")
    return dist2, index


def camera_table(cams) -> torch.Tensor:
    """The [C,16] fp32 HOST table `compute_filter_3D` takes, from FSGS-style cameras (`world_view_transform` = the transposed
    world-to-view matrix, `FoVx` / `FoVy`, `image_width` / `image_height`): per camera the 12 entries of [R | t] row by row, then
    fx, fy, W, H (include/syn3r_hip.h).  One device -> host read per camera: build it when the camera list changes, not per step."""
    import math
    rows = []
    for c in cams:
        w2c = c.world_view_transform.detach().to("cpu", torch.float32).t()
        W, H = float(c.image_width), float(c.image_height)
        fx, fy = W / (2.0 * math.tan(c.FoVx * 0.5)), H / (2.0 * math.tan(c.FoVy * 0.5))
        rows.append(torch.cat([w2c[:3, :].reshape(-1), torch.tensor([fx, fy, W, H], dtype=torch.float32)]))
    return torch.stack(rows) if rows else torch.zeros((0, 16), dtype=torch.float32)


def compute_filter_3D(xyz: torch.Tensor, cam_table: torch.Tensor, variance: float = L.FILTER3D_VARIANCE, near: float = L.FILTER3D_NEAR,
                      margin: float = L.FILTER3D_MARGIN) -> torch.Tensor:
    """Mip-Splatting's 3D smoothing filter size per Gaussian (`syn3r_filter3d_compute`, csrc/filter3d.hip): [N] fp32,
    sqrt(variance) / (max over the cameras that see the Gaussian of fx / z); unseen Gaussians take the largest filter among the
    seen ones, all zero when none is seen.  `xyz` [N,3] and `cam_table` [C,16] (`camera_table`) are fp32 DEVICE tensors.  Two
    launches on the current stream: no host read, no synchronisation.  The constants are RECALLED from the released code: UNPINNED."""
    dev = L.require_gpu(xyz, cam_table)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or cam_table.dim() != 2 or cam_table.shape[1] != 16:
        raise ValueError(f"compute_filter_3D: xyz must be [N,3] and cam_table [C,16], got {tuple(xyz.shape)} and {tuple(cam_table.shape)}")
    pts = xyz.detach().to(torch.float32).contiguous()
    tab = cam_table.detach().to(torch.float32).contiguous()
    n = pts.shape[0]
    lib = L.load()
    out = torch.empty(n, dtype=torch.float32, device=dev)
    ws = L.workspace(dev, lib.syn3r_filter3d_workspace_bytes(n), "filter3d")
    L.check(lib.syn3r_filter3d_compute(L.ptr(pts), n, L.ptr(tab), int(tab.shape[0]), float(variance), float(near), float(margin),
                                       L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr(dev)), "filter3d_compute")
    return out


def proximity_unpool(xyz: torch.Tensor, log_scales: torch.Tensor, opacity_logits: torch.Tensor, confidence: torch.Tensor,
                     score_thresh: float, log_scale_thresh: float) -> dict:
    """FSGS' proximity-guided Gaussian unpooling (Zhu et al., ECCV 2024, section 3.2) on raw parameters: Gaussian i is a source when the
    mean squared distance to its 3 nearest neighbours exceeds `score_thresh` and its largest log-scale exceeds `log_scale_thresh`
    (-inf: off); every source grows one Gaussian at the midpoint of each of its three graph edges, with the DESTINATION's log-scales,
    opacity logit and confidence and the identity rotation; SH coefficients of new Gaussians are zero (the caller's).  Sources in
    ascending index order, neighbours nearest first: bitwise repeatable.  FSGS' source is not available - the score (simple-knn's
    squared quantity), the scale test and the thresholds are UNPINNED, hence arguments.
    Returns {"xyz" [M,3], "scaling" [M,3] (log), "opacity" [M] (logit), "rotation" [M,4], "confidence" [M], "count": M = 3 S,
    "sources": S}.  ONE host read (S) between the count and the emit launches; S = 0 launches no emit."""
    pts = _cloud_arg("proximity_unpool", xyz)
    L.require_gpu(pts, log_scales, opacity_logits, confidence)
    n, dev = pts.shape[0], pts.device
    f32 = lambda t: t.detach().contiguous()
    ls, op, conf = f32(log_scales), f32(opacity_logits).reshape(-1), f32(confidence).reshape(-1)
    if ls.shape != (n, 3) or op.shape != (n,) or conf.shape != (n,) or any(t.dtype != torch.float32 for t in (ls, op, conf)):
        raise ValueError(f"proximity_unpool: float32 log_scales [n,3], opacity_logits [n] and confidence [n] for n={n} points; got "
                         f"{tuple(log_scales.shape)}, {tuple(opacity_logits.shape)}, {tuple(confidence.shape)}")
    lib = L.load()
    dist2, index = knn3_graph(pts)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws = L.workspace(dev, lib.syn3r_gaussian_unpool_workspace_bytes(n), "unpool")
    L.check(lib.syn3r_gaussian_unpool_count(L.ptr(dist2), L.ptr(ls), n, float(score_thresh), float(log_scale_thresh), L.ptr(count),
                                            L.ptr(ws), ws.numel(), L.stream_ptr(dev)), "gaussian_unpool_count")
    S = int(count.item())                                  # the one synchronisation
    M = 3 * S
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = {"xyz": new(M, 3), "scaling": new(M, 3), "opacity": new(M), "rotation": new(M, 4), "confidence": new(M),
           "count": M, "sources": S}
    if S > 0:
        L.check(lib.syn3r_gaussian_unpool_emit(L.ptr(pts), L.ptr(ls), L.ptr(op), L.ptr(conf), L.ptr(index), n, S, M, L.ptr(out["xyz"]),
                                               L.ptr(out["scaling"]), L.ptr(out["opacity"]), L.ptr(out["rotation"]),
                                               L.ptr(out["confidence"]), L.ptr(ws), ws.numel(), L.stream_ptr(dev)),
                "gaussian_unpool_emit")
    return out
