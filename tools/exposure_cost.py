"""What the per-camera affine exposure (`OptimizationParams.exposure_opt`: syn3r_exposure_apply / syn3r_exposure_backward + one
syn3r_adam_step on 12 floats) costs on the bench scene (developer tool; profiles/r15/exposure.txt).

    python tools/exposure_cost.py [--iters 200] [--rounds 3]

    1. the three kernels per launch on a render-sized image (and k_adam on 12 floats): the library's own kernel trace (event
       timestamps on the dispatch packets), 50 calls after 10, with the bytes each moves and the rate that makes
    2. the trainer's explicit step (GSTrainer.train_step: raw-parameter render, fused photometric loss, backward, fused Adam) on a
       pseudo-view with the option off / on, alternating: iterations per second, every step of the `on` trainer on an eligible camera"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import _devlib  # noqa: E402,F401  (SYN3R_LIB_OVERRIDE=<other build>: explicit, tool-side)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
mine = ap.parse_args()
sys.argv = sys.argv[:1]
args = bench.parse()

from syn3r_amd import _lib as L  # noqa: E402
from syn3r_amd import raster  # noqa: E402
from syn3r_amd import synthetic  # noqa: E402
from syn3r_amd.gs import Camera, GaussianModel, GSTrainer, OptimizationParams  # noqa: E402
from syn3r_amd.gs import train_ops as T  # noqa: E402

dev = torch.device("cuda", 0)
loop = bench.RasterLoop(args, dev)
H, W, N = args.height, args.width, args.gaussians
print(f"scene: {N} Gaussians, {H}x{W}; {mine.iters} iterations per timing, {mine.rounds} rounds, off / on alternating")

print("== 1. exposure kernels, us per launch (kernel trace, 50 calls)")
gen = torch.Generator().manual_seed(3)
image, grad_out = torch.rand(3, H, W, generator=gen).to(dev), torch.randn(3, H, W, generator=gen).to(dev)
A = (torch.eye(3, 4) + 0.05 * torch.randn(3, 4, generator=gen)).reshape(12).to(dev)
grad_A, m, v = torch.zeros(12, device=dev), torch.zeros(12, device=dev), torch.zeros(12, device=dev)
lib = L.load()


def once(step):
    T.exposure_apply_step(image, A)
    T.exposure_backward_step(image, A, grad_out, grad_A)
    L.check(lib.syn3r_adam_step(L.ptr(A), L.ptr(grad_A), L.ptr(m), L.ptr(v), 12, 0.0, 0.9, 0.999, 1e-15, step, L.stream_ptr(dev)), "adam_step")


for k in range(10):
    once(k + 1)
torch.cuda.synchronize()
with L.kernel_trace() as tr:
    for k in range(50):
        once(k + 11)
    torch.cuda.synchronize()
moved = {"k_exposure_apply": 24 * H * W, "k_exposure_pass": 36 * H * W}
for name, (calls, ms) in sorted(tr.result.items()):
    us = ms / calls * 1e3
    rate = f"   {moved[name] / 1e6:7.1f} MB   {moved[name] / (us * 1e-6) / 1e12:5.2f} TB/s" if name in moved else ""
    print(f"  {name:<20} calls {calls:4d}   avg {us:8.2f} us{rate}")

print("== 2. trainer explicit step on a pseudo-view (0.8 L1 + 0.2 (1 - SSIM), fused Adam; density control off), iterations per second")
fx = W / (2 * np.tan(np.deg2rad(60.0) / 2))
K = np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], dtype=np.float32)
pose = np.eye(4, dtype=np.float32)
g_m, g_s, g_q, g_o, g_sh = synthetic.synthetic_gaussians(N, seed=args.seed)
logit = torch.log(g_o.clamp(1e-3, 1 - 1e-3) / (1 - g_o.clamp(1e-3, 1 - 1e-3)))
# FSGS's learning rates x 1e-3, as bench.RasterLoop.full_iteration_rate: the target is noise, the timing should be of a steady scene
rates = dict(position_lr=1.6e-7, feature_lr=2.5e-6, opacity_lr=5e-5, scaling_lr=5e-6, rotation_lr=1e-6)
trainers, pseudo = {}, {}
for on in (False, True):
    gm = GaussianModel(g_m, torch.log(g_s), g_q, logit, g_sh, device=dev)
    cam = Camera.from_w2c(pose, K, H, W, image=loop.target.cpu(), data_device=dev)
    trainers[on] = GSTrainer(gm, [cam], OptimizationParams(exposure_opt=on, **rates))
    trainers[on].update_cameras([loop.target], [pose], K, 1.0)
    pseudo[on] = trainers[on].pseudo_cameras[0]
raster.set_pair_count_mode("sync")
for on in (False, True):
    with torch.no_grad():
        trainers[on].render_view(pseudo[on])              # seeds the async pair capacity of the shape
raster.set_pair_count_mode("async")
for on in (False, True):
    for _ in range(10):
        trainers[on].train_step(pseudo[on])
torch.cuda.synchronize()
for r in range(mine.rounds):
    row = []
    for on in (False, True):
        t0 = time.perf_counter()
        for _ in range(mine.iters):
            trainers[on].train_step(pseudo[on])
        torch.cuda.synchronize()
        row.append(mine.iters / (time.perf_counter() - t0))
    print(f"  round {r}: off {row[0]:.1f} /s   on {row[1]:.1f} /s   on/off {row[1] / row[0]:.4f}")
raster.flush_pair_checks()
assert trainers[True].exposure_updates == 10 + mine.rounds * mine.iters and trainers[False].exposure_updates == 0
