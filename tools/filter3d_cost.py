"""What Mip-Splatting's 3D smoothing filter (`OptimizationParams.filter_3d`, syn3r_filter3d_compute / syn3r_raster_*_f3d) costs on the
bench scene (developer tool; profiles/r11/raster_filter3d.txt).

    python tools/filter3d_cost.py [--iters 200] [--rounds 3] [--cameras 25]

    1. k_preprocess / k_preprocess_bwd per launch, filter off / on (the library's own kernel trace: event timestamps on the dispatch
       packets; each mode traced in a run of its own, since both instances carry the one trace name)
    2. raster fwd+bwd iteration, filter off / on alternating, host clock around a synchronised loop
    3. syn3r_filter3d_compute at the scene's Gaussians x --cameras cameras: traced kernels and the host clock around a synchronised loop
    4. the trainer's explicit step (GSTrainer.train_step: raw-parameter render, fused photometric loss, backward, fused Adam) with the
       option off / on, --cameras training cameras, filter_3d_interval at its default: iterations per second
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--cameras", type=int, default=25)
mine = ap.parse_args()
sys.argv = sys.argv[:1]
args = bench.parse()

from syn3r_amd import _lib as L  # noqa: E402
from syn3r_amd import raster  # noqa: E402
from syn3r_amd import synthetic  # noqa: E402
from syn3r_amd.gs import Camera, GaussianModel, GSTrainer, OptimizationParams  # noqa: E402
from syn3r_amd.gs.train_ops import camera_table, compute_filter_3D  # noqa: E402
from syn3r_amd.raster import GaussianRasterizer  # noqa: E402

dev = torch.device("cuda", 0)
loop = bench.RasterLoop(args, dev)
H, W, N = args.height, args.width, args.gaussians
fx = W / (2 * np.tan(np.deg2rad(60.0) / 2))
K = np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], dtype=np.float32)


def pose(i):
    """camera i of a 5 x 5 fan in front of the scene (z in 2 .. 6), at three distances"""
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = (-0.2 * (i % 5 - 2), -0.2 * ((i // 5) % 5 - 2), 0.5 * (i % 3))
    return m


target = loop.target.cpu()
cams = [Camera.from_w2c(pose(i), K, H, W, image=target, data_device=dev) for i in range(mine.cameras)]
table = camera_table(cams).to(dev)
filt = compute_filter_3D(loop.p["m"], table)
torch.cuda.synchronize()
s_med = float(loop.p["s"].detach().median())
print(f"scene: {N} Gaussians, {H}x{W}, {mine.cameras} cameras; filter min / median / max {float(filt.min()):.5f} / {float(filt.median()):.5f} / "
      f"{float(filt.max()):.5f} (median scale {s_med:.5f}); {mine.iters} iterations per timing, {mine.rounds} rounds, off / on alternating")


class Filtered(GaussianRasterizer):
    def forward(self, *a, **kw):
        return super().forward(*a, filter_3D=filt, **kw)


rast = {False: GaussianRasterizer(loop.rast.raster_settings), True: Filtered(loop.rast.raster_settings)}


def run(on, n):
    loop.rast = rast[on]
    for _ in range(n):
        loop.iteration()
    torch.cuda.synchronize()


for on in (False, True):
    run(on, 10)
print("== 1. projection kernels, us per launch (kernel trace, 50 iterations per mode)")
for on in (False, True):
    with L.kernel_trace() as tr:
        run(on, 50)
    for name, (calls, ms) in sorted(tr.result.items()):
        if name.startswith("k_preprocess"):
            print(f"  filter {'on ' if on else 'off'}  {name:<26} calls {calls:4d}   avg {ms / calls * 1e3:8.2f} us")
print("== 2. raster fwd+bwd iteration (render, L1, backward; async pair-count mode)")
for r in range(mine.rounds):
    row = []
    for on in (False, True):
        t0 = time.perf_counter()
        run(on, mine.iters)
        row.append((time.perf_counter() - t0) / mine.iters * 1e3)
    print(f"  round {r}: off {row[0]:.4f} ms   on {row[1]:.4f} ms   on/off {row[1] / row[0]:.4f}")
raster.flush_pair_checks()

print(f"== 3. syn3r_filter3d_compute, {N} Gaussians x {mine.cameras} cameras")
with L.kernel_trace() as tr:
    for _ in range(50):
        compute_filter_3D(loop.p["m"], table)
    torch.cuda.synchronize()
for name, (calls, ms) in sorted(tr.result.items()):
    if name.startswith("k_filter3d"):
        print(f"  {name:<20} calls {calls:4d}   avg {ms / calls * 1e3:8.2f} us")
for r in range(mine.rounds):
    t0 = time.perf_counter()
    for _ in range(mine.iters):
        compute_filter_3D(loop.p["m"], table)
    torch.cuda.synchronize()
    print(f"  round {r}: {(time.perf_counter() - t0) / mine.iters * 1e6:.2f} us per call (memset + two launches, host clock, synchronised loop)")

print("== 4. trainer explicit step (0.8 L1 + 0.2 (1 - SSIM), fused Adam), iterations per second")
m, s, q, o, sh = synthetic.synthetic_gaussians(N, seed=args.seed)
logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
# FSGS's learning rates x 1e-3, as bench.RasterLoop.full_iteration_rate: the target is noise, the timing should be of a steady scene
rates = dict(position_lr=1.6e-7, feature_lr=2.5e-6, opacity_lr=5e-5, scaling_lr=5e-6, rotation_lr=1e-6)
trainers = {}
for on in (False, True):
    gm = GaussianModel(m, torch.log(s), q, logit, sh, device=dev)
    trainers[on] = GSTrainer(gm, cams, OptimizationParams(filter_3d=on, **rates))
raster.set_pair_count_mode("sync")
for on in (False, True):
    with torch.no_grad():
        for cam in cams:
            trainers[on].render_view(cam)          # seeds the async pair capacity of the shape (the largest view counts)
raster.set_pair_count_mode("async")
for on in (False, True):
    for _ in range(10):
        trainers[on].train_step()
torch.cuda.synchronize()
for r in range(mine.rounds):
    row = []
    for on in (False, True):
        tr_ = trainers[on]
        t0 = time.perf_counter()
        for _ in range(mine.iters):
            tr_.train_step()
        torch.cuda.synchronize()
        row.append(mine.iters / (time.perf_counter() - t0))
    print(f"  round {r}: off {row[0]:.1f} /s   on {row[1]:.1f} /s   on/off {row[1] / row[0]:.4f}   (filter computed {trainers[True].filter_3d_computes} times so far)")
raster.flush_pair_checks()
