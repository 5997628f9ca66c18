"""Cost of the edge-aware depth-smoothness term (csrc/depth_smooth.hip: k_dsmooth_weights, k_dsmooth_stats, k_dsmooth_grad) beside the
global depth-correlation step (developer tool; profiles/r20/depth_smooth.txt).

    python tools/depth_smooth_bench.py [--iters 500 | --iters 0] [--out profiles/r20/depth_smooth.txt]

    1. syn3r_depth_smooth_loss_step at 1920x1080 and 1024x576, accumulate 0 and 1: per kernel (the library's kernel trace: event
       timestamps on the dispatch packets) and per step (device events around 200 back-to-back calls, the gap between the two
       launches included), syn3r_depth_corr_loss_step the same way in the same run, and syn3r_depth_edge_weights (once per camera).
       The smoothness step moves 7 planes (the statistics pass reads d, wx, wy; the gradient pass reads them again and writes one),
       the correlation step 5.  Next to each kernel: the time its bytes alone allow at the rate a plain device copy of four
       planes (eight planes moved) reaches at this size in this run.  The bar: at 1080p the new step takes at most 1.75 x the
       correlation step of this run.
    2. GSTrainer.training() iterations / s at 200 000 Gaussians / 1080p with the term off and on, interleaved."""
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
from syn3r_amd.gs.train_ops import depth_correlation_loss_step, depth_edge_weights, depth_smoothness_loss_step

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--out", type=str, default=str(Path(__file__).resolve().parents[1] / "profiles" / "r20" / "depth_smooth.txt"))
args = ap.parse_args()
dev = torch.device("cuda", 0)
REPS = 200
BAR = 1.75
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
    image = torch.rand(3, H, W, generator=g).to(dev)
    plane = 4.0 * H * W / 1e6                                       # MB
    kern, glob = timed(lambda: depth_correlation_loss_step(d, p, 0.05), "k_dcorr")
    src, dst = torch.rand(4, H, W, device=dev), torch.empty(4, H, W, device=dev)
    _, copy = timed(lambda: dst.copy_(src), "k_none")
    rate = 8 * plane / copy                                         # TB/s of a plain copy at this size
    say(f"  {W}x{H}  (one plane {plane:.1f} MB; a device copy of 4 planes takes {copy:.2f} us: {rate:.2f} TB/s)")
    say(f"    correlation  5 planes  " + "  ".join(f"{k} {v:7.2f}" for k, v in kern.items()) + f"   step {glob:7.2f}   {5 * plane / glob:5.2f} TB/s")
    kw, once = timed(lambda: depth_edge_weights(image, 1.0), "k_dsmooth")
    say(f"    edge weights 5 planes  " + "  ".join(f"{k} {v:7.2f}" for k, v in kw.items()) + f"   call {once:7.2f}   (once per camera; "
        f"{8.0 * H * W / 1e6:.1f} MB kept per camera)")
    w = depth_edge_weights(image, 1.0)
    buf = torch.zeros(1, H, W, device=dev)
    for acc, planes in ((0, {"k_dsmooth_stats": 3, "k_dsmooth_grad": 4}), (1, {"k_dsmooth_stats": 3, "k_dsmooth_grad": 5})):
        kern, step = timed(lambda: depth_smoothness_loss_step(d, w, 0.05, grad_out=buf if acc else None), "k_dsmooth")
        total = sum(planes.values())
        verdict = ""
        if (H, W) == (1080, 1920) and acc == 0:
            verdict = f"   bar {BAR}: " + ("met" if step <= BAR * glob else f"MISSED by {step / glob - BAR:.2f}")
        say(f"    smoothness acc={acc} {total} planes  " +
            "  ".join(f"{k} {v:7.2f} (bytes alone {planes.get(k, 0) * plane / rate:5.2f})" for k, v in kern.items()) +
            f"   step {step:7.2f}   {total * plane / step:5.2f} TB/s   smoothness / correlation {step / glob:5.2f}{verdict}")

if args.iters > 0:                                              # (--iters 0: the step entries alone)
    say(f"== 2. GSTrainer.training(), 200 000 Gaussians, 1920x1080, iterations / s over {args.iters} iterations, off / on interleaved")
    N, H, W = 200_000, 1080, 1920
    with tempfile.TemporaryDirectory() as tmp:
        tr = measure.synthetic_scene(dev, N, H, W, 2, args.iters + 1, tmp)        # (+ 1: no checkpoint inside a timed window)
        rates = {0.0: [], 0.05: []}
        for sw in (0.0, 0.05, 0.0, 0.05, 0.0, 0.05):            # interleaved: box drift shows as a spread, not as a bias
            tr.opt.depth_smooth_weight = sw
            tr.training(0, iterations=50, disable_densification=True)      # warm-up: capacities, workspaces, the cameras' edge weights
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.training(0, iterations=args.iters, disable_densification=True)
            torch.cuda.synchronize()
            rates[sw].append(args.iters / (time.perf_counter() - t0))
    for k, (a, b) in enumerate(zip(rates[0.0], rates[0.05])):
        say(f"  round {k}: off {a:.1f} /s   on {b:.1f} /s   on/off {b / a:.4f}   (+{(1 / b - 1 / a) * 1e6:.1f} us per step)")
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text("\n".join(lines) + "\n")
