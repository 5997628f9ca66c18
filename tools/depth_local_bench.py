"""Cost of the patch-wise depth-correlation term (csrc/depth_loss.hip: k_dlocal_stats, k_dlocal_grad) beside the global one
(developer tool; profiles/r19/depth_local.txt).

    python tools/depth_local_bench.py [--iters 500] [--out profiles/r19/depth_local.txt]

    1. syn3r_depth_corr_local_loss_step at 1920x1080 and 1024x576 for P in {8, 16, 32, 64, 256}, origin (5, 3): per kernel (the
       library's kernel trace: event timestamps on the dispatch packets) and per step (device events around 200 back-to-back calls,
       the gap between the two launches included), and the global syn3r_depth_corr_loss_step the same way in the same run.  Both
       move d and p twice and the gradient once: 20 bytes per pixel.  The bar: at 1080p, P in {16, 32, 64}, a local step takes at
       most 1.5 x the global step of this run.
    2. GSTrainer.training() iterations / s at 200 000 Gaussians / 1080p with the term off and on (P = 32, jittered origin), interleaved;
       the priors are the truth cloud's disparities."""
import argparse
import sys
import tempfile
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import _devlib  # noqa: F401  (SYN3R_LIB_OVERRIDE=<other build>: explicit, tool-side)
from syn3r_amd import _lib as L
from syn3r_amd import measure
from syn3r_amd.gs import GaussianModel, GSTrainer
from syn3r_amd.gs.train_ops import depth_correlation_local_loss_step, depth_correlation_loss_step
from syn3r_amd.launch import truth_disparity
from syn3r_amd.synthetic import synthetic_gaussians

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--out", type=str, default=str(Path(__file__).resolve().parents[1] / "profiles" / "r19" / "depth_local.txt"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
PATCHES = (8, 16, 32, 64, 256)
BARRED = (16, 32, 64)
REPS = 200
lines = []


def say(text: str):
    print(text, flush=True)
    lines.append(text)


def timed(call, only):
    """-> ({kernel: us per launch}, us per call on the stream)"""
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    with L.kernel_trace(only=only) as tr_:
        for _ in range(REPS):
            call()
        torch.cuda.synchronize()
    kern = {k: 1000.0 * ms / c for k, (c, ms) in sorted(tr_.result.items())}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        call()
    e1.record()
    torch.cuda.synchronize()
    return kern, 1000.0 * e0.elapsed_time(e1) / REPS


say(f"== 1. the step entries, us (kernel trace per launch; stream time per call over {REPS} back-to-back calls)")
for H, W in ((1080, 1920), (576, 1024)):
    g = torch.Generator().manual_seed(0)
    d = (20.0 + torch.rand(1, H, W, generator=g)).to(dev)
    p = (1.0 / d[0] + 0.01 * torch.rand(H, W, generator=g).to(dev)).contiguous()
    mb = 20.0 * H * W / 1e6
    kern, glob = timed(lambda: depth_correlation_loss_step(d, p, 0.05), "k_dcorr")
    say(f"  {W}x{H}  ({mb:.1f} MB moved per step)")
    say(f"    global            " + "  ".join(f"{k} {v:7.2f}" for k, v in kern.items()) + f"   step {glob:7.2f}   {mb / glob:5.2f} TB/s")
    for P in PATCHES:
        kern, loc = timed(lambda: depth_correlation_local_loss_step(d, p, 0.05, P, (5, 3)), "k_dlocal")
        K = ((H - 5) // P) * ((W - 3) // P)
        verdict = ""
        if (H, W) == (1080, 1920) and P in BARRED:
            verdict = "   bar 1.5: " + ("met" if loc <= 1.5 * glob else f"MISSED by {loc / glob - 1.5:.2f}")
        say(f"    local P={P:<3} K={K:<6}" + "  ".join(f"{k} {v:7.2f}" for k, v in kern.items()) +
            f"   step {loc:7.2f}   {mb / loc:5.2f} TB/s   local / global {loc / glob:5.2f}{verdict}")

say(f"== 2. GSTrainer.training(), 200 000 Gaussians, 1920x1080, iterations / s over {args.iters} iterations, off / on interleaved")
N, H, W = 200_000, 1080, 1920
m, s, q, o, sh = synthetic_gaussians(N, seed=0)
logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
truth = GSTrainer(GaussianModel(m, torch.log(s), q, logit, sh, device=dev), [])
with tempfile.TemporaryDirectory() as tmp:
    tr = measure.synthetic_scene(dev, N, H, W, 2, args.iters + 1, tmp)        # (+ 1: no checkpoint inside a timed window)
    for cam in tr.scene.getTrainCameras():
        cam.depth_image = truth_disparity(truth, cam)
    del truth
    tr.opt.depth_patch_size = 32
    rates = {0.0: [], 0.05: []}
    for dw in (0.0, 0.05, 0.0, 0.05, 0.0, 0.05):            # interleaved: box drift shows as a spread, not as a bias
        tr.opt.depth_local_weight = dw
        tr.training(0, iterations=50, disable_densification=True)      # warm-up: capacities, workspaces
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.training(0, iterations=args.iters, disable_densification=True)
        torch.cuda.synchronize()
        rates[dw].append(args.iters / (time.perf_counter() - t0))
for k, (a, b) in enumerate(zip(rates[0.0], rates[0.05])):
    say(f"  round {k}: off {a:.1f} /s   on {b:.1f} /s   on/off {b / a:.4f}   (+{(1 / b - 1 / a) * 1e6:.1f} us per step)")
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text("\n".join(lines) + "\n")
