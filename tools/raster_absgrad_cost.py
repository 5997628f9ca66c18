"""What AbsGS' absolute screen-space gradient (`OptimizationParams.densify_abs_grad`, syn3r_raster_backward_abs: the ABS instances of
k_render_bwd + k_abs_means2D) costs on the bench scene (developer tool; profiles/r13/raster_absgrad.txt).

    python tools/raster_absgrad_cost.py [--iters 200] [--rounds 3] [--off-only]

    1. the backward's kernels per launch, option off / on, without and with a depth gradient (both HAS_DEPTH_GRAD instances): the
       library's own kernel trace (event timestamps on the dispatch packets); each mode traced in a run of its own, since the four
       instances of k_render_bwd carry the one trace name.  One forward, then the backward alone, over and over
    2. raster fwd+bwd iteration (bench.RasterLoop: render, L1, autograd backward), option off / on alternating, host clock around a
       synchronised loop
    3. the trainer's explicit step (GSTrainer.train_step: raw-parameter render, fused photometric loss, backward, fused Adam) with the
       option off / on: iterations per second

--off-only: sections 1 to 3 with the option off alone - runs against a build without the entry (SYN3R_LIB_OVERRIDE=<the parent
commit's library>: the same box, the same scene, the parent's kernel)."""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import _devlib  # noqa: E402,F401  (SYN3R_LIB_OVERRIDE=<other build>: explicit, tool-side)
import torch  # noqa: E402

import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--off-only", action="store_true")
mine = ap.parse_args()
sys.argv = sys.argv[:1]
args = bench.parse()

from syn3r_amd import _lib as L  # noqa: E402
from syn3r_amd import raster  # noqa: E402
from syn3r_amd import synthetic  # noqa: E402
from syn3r_amd.gs import Camera, GaussianModel, GSTrainer, OptimizationParams  # noqa: E402
from syn3r_amd.raster import GaussianRasterizer, rasterize_backward, rasterize_forward  # noqa: E402

if mine.off_only:                    # a library without the `_abs` entries: bind what it has
    for name in ("syn3r_raster_backward_abs", "syn3r_densification_stats_abs"):
        L.SIGNATURES.pop(name, None)

dev = torch.device("cuda", 0)
loop = bench.RasterLoop(args, dev)
H, W, N = args.height, args.width, args.gaussians
modes = (False,) if mine.off_only else (False, True)
print(f"scene: {N} Gaussians, {H}x{W}; {mine.iters} iterations per timing, {mine.rounds} rounds, off / on alternating"
      + ("  [option off only]" if mine.off_only else ""))

print("== 1. backward kernels, us per launch (kernel trace, 50 backwards per mode)")
raster.set_pair_count_mode("sync")
p = {k: v.detach() for k, v in loop.p.items()}
with torch.no_grad():
    color, radii, depth, alpha, st = rasterize_forward(p["m"], p["sh"], p["o"], p["s"], p["q"], None, loop.rast.raster_settings)
    gen = torch.Generator().manual_seed(3)
    g_color, g_depth = torch.randn(3, H, W, generator=gen).to(dev), torch.randn(1, H, W, generator=gen).to(dev)
    buf = torch.empty(N, 2, device=dev)
    for with_depth in (False, True):
        for on in modes:
            kw = dict(abs_grad_out=buf) if on else {}
            back = lambda: rasterize_backward(st, g_color, g_depth if with_depth else None, **kw)
            for _ in range(10):
                back()
            torch.cuda.synchronize()
            with L.kernel_trace() as tr:
                for _ in range(50):
                    back()
                torch.cuda.synchronize()
            for name, (calls, ms) in sorted(tr.result.items()):
                print(f"  depth gradient {'yes' if with_depth else 'no '}  option {'on ' if on else 'off'}  {name:<26} calls {calls:4d}"
                      f"   avg {ms / calls * 1e3:8.2f} us")
    if not mine.off_only:
        plain = rasterize_backward(st, g_color, g_depth)[1][:, :2].norm(dim=1)
        hit = plain > 0
        print(f"  abs gradient: {int((radii > 0).sum())} visible Gaussians, {int(hit.sum())} with a non-zero plain gradient; over those, median "
              f"|abs| / |plain| = {float((buf.norm(dim=1)[hit] / plain[hit]).median()):.2f}")
del st
raster.set_pair_count_mode("async")


class WithAbs(GaussianRasterizer):
    def forward(self, *a, **kw):
        return super().forward(*a, means2D_abs=buf, **kw)


rast = {False: GaussianRasterizer(loop.rast.raster_settings), True: WithAbs(loop.rast.raster_settings)}


def run(on, n):
    loop.rast = rast[on]
    for _ in range(n):
        loop.iteration()
    torch.cuda.synchronize()


for on in modes:
    run(on, 10)
print("== 2. raster fwd+bwd iteration (render, L1, backward; async pair-count mode)")
for r in range(mine.rounds):
    row = []
    for on in modes:
        t0 = time.perf_counter()
        run(on, mine.iters)
        row.append((time.perf_counter() - t0) / mine.iters * 1e3)
    print(f"  round {r}: off {row[0]:.4f} ms" + (f"   on {row[1]:.4f} ms   on/off {row[1] / row[0]:.4f}" if len(row) > 1 else ""))
raster.flush_pair_checks()

print("== 3. trainer explicit step (0.8 L1 + 0.2 (1 - SSIM), fused Adam; density control off), iterations per second")
import numpy as np  # noqa: E402
fx = W / (2 * np.tan(np.deg2rad(60.0) / 2))
K = np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], dtype=np.float32)
cam = Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, image=loop.target.cpu(), data_device=dev)
m, s, q, o, sh = synthetic.synthetic_gaussians(N, seed=args.seed)
logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
# FSGS's learning rates x 1e-3, as bench.RasterLoop.full_iteration_rate: the target is noise, the timing should be of a steady scene
rates = dict(position_lr=1.6e-7, feature_lr=2.5e-6, opacity_lr=5e-5, scaling_lr=5e-6, rotation_lr=1e-6)
trainers = {}
for on in modes:
    gm = GaussianModel(m, torch.log(s), q, logit, sh, device=dev)
    trainers[on] = GSTrainer(gm, [cam], OptimizationParams(**(dict(densify_abs_grad=True) if on else {}), **rates))
raster.set_pair_count_mode("sync")
for on in modes:
    with torch.no_grad():
        trainers[on].render_view(cam)              # seeds the async pair capacity of the shape
raster.set_pair_count_mode("async")
for on in modes:
    for _ in range(10):
        trainers[on].train_step()
torch.cuda.synchronize()
for r in range(mine.rounds):
    row = []
    for on in modes:
        tr_ = trainers[on]
        t0 = time.perf_counter()
        for _ in range(mine.iters):
            tr_.train_step()
        torch.cuda.synchronize()
        row.append(mine.iters / (time.perf_counter() - t0))
    print(f"  round {r}: off {row[0]:.1f} /s" + (f"   on {row[1]:.1f} /s   on/off {row[1] / row[0]:.4f}" if len(row) > 1 else ""))
raster.flush_pair_checks()
