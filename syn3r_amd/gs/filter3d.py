"""What the trainer keeps between steps for Mip-Splatting's 3D smoothing filter (`OptimizationParams.filter_3d`): the camera table of
`train_ops.compute_filter_3D`, the camera list it was built from and the filter's age."""
from __future__ import annotations

from typing import Optional

import torch

from .train_ops import camera_table, compute_filter_3D


class Filter3DCache:
    def __init__(self):
        self.cams, self.length, self.table, self.age = None, -1, None, 0
        self.computes = 0                 # how often `ensure` has computed the filter

    def tick(self):
        """One optimisation step has moved the positions."""
        self.age += 1

    def invalidate_cameras(self):
        """Registered cameras have moved (pose refinement, a restored checkpoint): the next `ensure` builds the table again."""
        self.table = None

    def ensure(self, g, o, cams) -> Optional[torch.Tensor]:
        """`opt.filter_3d`: keep `gaussians.filter_3D` (Mip-Splatting's 3D smoothing filter, `train_ops.compute_filter_3D`) current and
        return it; None with the option off (nothing is touched).  Called at the top of every step and of `render_view`.  The
        filter is computed again when it is missing or its length is not N (clone, split, unpooling, prune, `set_from_pcd`,
        `restore`), when the camera list `scene.train_cameras[1.0]` is another object or has another length (`update_cameras`, the
        orchestrator's restore), or after `opt.filter_3d_interval` optimisation steps (positions move).  The cameras are ALL
        registered ones, pseudo-views included while they are registered; the view being rendered plays no part - rendering from a
        camera that did not train the Gaussians must not adapt them to it.  The [C,16] camera table is built (one host read per
        camera) and uploaded only when the list changes; the computation itself is two launches with no host synchronisation, so
        the training loop stays free of round trips.  No cameras: all-zero filters.
        `g`: the GaussianModel, `o`: the OptimizationParams, `cams`: `scene.train_cameras[1.0]`."""
        if not o.filter_3d:
            return None
        n, dev = g._xyz.shape[0], g._xyz.device
        stale = g.filter_3D is None or g.filter_3D.shape[0] != n or self.age >= max(int(o.filter_3d_interval), 1)
        if self.cams is not cams or self.length != len(cams) or self.table is None or self.table.device != dev:
            self.cams, self.length = cams, len(cams)                     # (the reference keeps the list alive: no recycled id)
            self.table = camera_table(cams).to(dev)
            stale = True
        if stale:
            if len(cams) == 0:
                g.filter_3D = torch.zeros(n, dtype=torch.float32, device=dev)
            else:
                g.filter_3D = compute_filter_3D(g._xyz, self.table, variance=float(o.filter_3d_variance))
            self.age = 0
            self.computes += 1
        return g.filter_3D
