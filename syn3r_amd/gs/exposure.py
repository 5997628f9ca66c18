"""Per-camera affine exposure compensation, host side (EXTENSION: the reference has none, nothing reference-held pins any of this).

A diffusion pseudo-view drifts in brightness, white balance and contrast against the input photographs, and captured views differ among
themselves through auto-exposure.  With `OptimizationParams.exposure_opt` an eligible camera holds a 3 x 4 matrix A, initialised to
[I | 0], and its loss compares E(render) with the camera's target:

    E_c(p) = A[c][0] I_0(p) + A[c][1] I_1(p) + A[c][2] I_2(p) + A[c][3]            (added left to right, no clamp)

The convention (3 x 3 block times the colour as a column, then the offset) is this repository's; the published 3DGS code multiplies a
row vector by the transposed block - recalled, UNPINNED.  The kernels are `syn3r_exposure_apply` / `syn3r_exposure_backward`
(csrc/exposure.hip) behind `train_ops.exposure_apply[_step]` / `exposure_backward_step`, the update is `syn3r_adam_step` on the 12
floats.  The state lives on the camera object - `cam.exposure` (device [12]) and `cam.exposure_adam` ({"m", "v"} device [12], "t" a host
int) - so it survives `update_cameras` and the orchestrator's restoring of the camera list.  No host read in a step.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib as L
from .params import expon_lr
from .train_ops import exposure_apply_step, exposure_backward_step

CAMERA_KINDS = ("pseudo", "train", "all")
BETAS, EPS = (0.9, 0.999), 1e-15          # recalled from the released 3DGS exposure optimiser: UNPINNED
IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


class ExposureControl:
    """The trainer's side of `OptimizationParams.exposure_opt`: which cameras have an exposure, their state, the [12] gradient buffer
    of the explicit route and the Adam step.  It reads the trainer's `opt`, `scene`, `iteration` and `gaussians` (for the device) when it
    needs them, never at construction."""

    def __init__(self, trainer):
        self.trainer = trainer
        self.updates = 0                  # exposure steps taken so far (`step`)
        self.grad = None                  # device [12]: d loss / d A of the explicit route's current step

    def eligible(self, cam) -> bool:
        """The option on and the camera of the chosen kind; for "train" and "all" not the first training camera (the gauge: with every
        camera free a global colour change costs nothing)."""
        o = self.trainer.opt
        if not o.exposure_opt:
            return False
        pseudo = bool(getattr(cam, "is_pseudo", False))
        if (pseudo and o.exposure_cameras == "train") or (not pseudo and o.exposure_cameras == "pseudo"):
            return False
        if not pseudo:
            train = self.trainer.scene.getTrainCameras()
            if train and train[0] is cam:
                return False
        return True

    def state(self, cam) -> Optional[torch.Tensor]:
        """`cam.exposure` of an eligible camera, created as the identity with a zero Adam state at its first step; None for a camera
        that runs the plain step."""
        if not self.eligible(cam):
            return None
        if getattr(cam, "exposure", None) is None:
            dev = self.trainer.gaussians._xyz.device
            cam.exposure = torch.tensor(IDENTITY, dtype=torch.float32, device=dev)
            cam.exposure_adam = {"m": torch.zeros(12, dtype=torch.float32, device=dev),
                                 "v": torch.zeros(12, dtype=torch.float32, device=dev), "t": 0}
        return cam.exposure

    def lr(self) -> float:
        """`exposure_lr`, or with `exposure_lr_final` set the published log-linear decay at the loop's 1-based step counter (the counter
        `GSTrainer.update_learning_rate` takes)."""
        o = self.trainer.opt
        if o.exposure_lr_final is None:
            return float(o.exposure_lr)
        return expon_lr(self.trainer.iteration + 1, float(o.exposure_lr), float(o.exposure_lr_final),
                        max_steps=int(o.exposure_lr_max_steps))

    def exposed(self, image: torch.Tensor, cam) -> torch.Tensor:
        """E(image) for a camera that has an exposure, else `image` itself"""
        A = getattr(cam, "exposure", None)
        return image if A is None else exposure_apply_step(image, A)

    def backward(self, image: torch.Tensor, cam, grad_out: torch.Tensor) -> torch.Tensor:
        """The explicit route: d loss / d E(image) -> d loss / d image; d loss / d A is left in `self.grad` (`step` reads it)."""
        if self.grad is None or self.grad.device != image.device:
            self.grad = torch.zeros(12, dtype=torch.float32, device=image.device)
        return exposure_backward_step(image, cam.exposure, grad_out, self.grad)

    @torch.no_grad()
    def step(self, cam, grad: Optional[torch.Tensor] = None):
        """One Adam step on `cam.exposure` (`syn3r_adam_step`, t += 1) with `grad` [12] (default: the buffer `backward` filled).
        Independent of the density control: the gradient belongs to the camera, whatever happened to the Gaussians."""
        grad = self.grad if grad is None else grad.detach().reshape(12).contiguous()
        A, st = cam.exposure, cam.exposure_adam
        dev = L.require_gpu(A, grad, st["m"], st["v"])
        st["t"] = int(st["t"]) + 1
        L.check(L.load().syn3r_adam_step(L.ptr(A), L.ptr(grad), L.ptr(st["m"]), L.ptr(st["v"]), 12, self.lr(), BETAS[0], BETAS[1], EPS,
                                         st["t"], L.stream_ptr(dev)), "adam_step (exposure)")
        self.updates += 1

    def capture(self) -> list:
        """Per registered camera that has state: index, kind, A and the Adam state (the checkpoint loader reads tensors and ints only)"""
        out = []
        for i, cam in enumerate(self.trainer.scene.train_cameras[1.0]):
            A, st = getattr(cam, "exposure", None), getattr(cam, "exposure_adam", None)
            if A is None or st is None:
                continue
            out.append({"index": i, "is_pseudo": int(bool(getattr(cam, "is_pseudo", False))), "A": A.detach().clone(),
                        "m": st["m"].detach().clone(), "v": st["v"].detach().clone(), "t": int(st["t"])})
        return out

    def restore(self, entries: list):
        """Entry i goes to registered camera i when there is one of the same kind (a checkpoint written with pseudo-views registered
        may be loaded after the list was restored: their entries are skipped)."""
        cams = self.trainer.scene.train_cameras[1.0]
        dev = self.trainer.gaussians._xyz.device
        put = lambda t: t.detach().to(dev, torch.float32).reshape(12).contiguous().clone()
        for e in entries:
            i = int(e["index"])
            if i >= len(cams) or int(bool(getattr(cams[i], "is_pseudo", False))) != int(e["is_pseudo"]):
                continue
            cams[i].exposure = put(e["A"])
            cams[i].exposure_adam = {"m": put(e["m"]), "v": put(e["v"]), "t": int(e["t"])}
