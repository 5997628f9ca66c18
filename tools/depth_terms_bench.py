"""Cost of one of the trainer's three depth terms (developer tool): the global depth correlation and the patch-wise one
(csrc/depth_loss.hip: k_dcorr_*, k_dlocal_*) and the edge-aware smoothness (csrc/depth_smooth.hip: k_dsmooth_*).

    python tools/depth_terms_bench.py --term {global,local,smooth} [--iters 500 | --iters 0] [--out FILE]

    1. The term's step entry at 1920x1080 and 1024x576: per kernel (the library's kernel trace: event timestamps on the dispatch
       packets) and per step (device events around 200 back-to-back calls, the gap between the two launches included), with
       syn3r_depth_corr_loss_step, the yardstick of the other two, the same way in the same run.
       global: that step alone; it moves d and p twice and the gradient once: 20 bytes per pixel.
       local:  P in {8, 16, 32, 64, 256}, origin (5, 3); the same 20 bytes per pixel.  The bar: at 1080p, P in {16, 32, 64}, a local
               step takes at most 1.5 x the global step of this run.
       smooth: accumulate 0 and 1, and syn3r_depth_edge_weights (once per camera).  The step moves 7 planes (the statistics pass
               reads d, wx, wy; the gradient pass reads them again and writes one), the correlation step 5.  Next to each kernel: the
               time its bytes alone allow at the rate a plain device copy of four planes (eight planes moved) reaches at this size
               in this run.  The bar: at 1080p the step takes at most 1.75 x the correlation step of this run.
    2. GSTrainer.training() iterations / s at 200 000 Gaussians / 1080p with the term off and on, interleaved (local: P = 32, jittered
       origin); where the term needs a prior, the priors are the truth cloud's disparities.  --iters 0: section 1 alone.
    --out defaults to profiles/r21/depth_global.txt, profiles/r19/depth_local.txt, profiles/r20/depth_smooth.txt; with --iters 0 and no
    --out nothing is written (a section-1 run does not replace a full record)."""
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
from syn3r_amd.gs.train_ops import (depth_correlation_local_loss_step, depth_correlation_loss_step, depth_edge_weights,
                                    depth_smoothness_loss_step)

# term -> (the option section 2 toggles, do its cameras need a prior, default --out under profiles/)
TERMS = {"global": ("depth_weight", True, "r21/depth_global.txt"), "local": ("depth_local_weight", True, "r19/depth_local.txt"),
         "smooth": ("depth_smooth_weight", False, "r20/depth_smooth.txt")}
ap = argparse.ArgumentParser()
ap.add_argument("--term", choices=sorted(TERMS), required=True)
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
option, needs_prior, default_out = TERMS[args.term]
out = Path(args.out or Path(__file__).resolve().parents[1] / "profiles" / default_out) if args.out or args.iters > 0 else None
dev = torch.device("cuda", 0)
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


def cols(kern, extra=lambda k: ""):
    return "  ".join(f"{k} {v:7.2f}{extra(k)}" for k, v in kern.items())


def local_rows(d, p, H, W, mb, glob):
    for P in (8, 16, 32, 64, 256):
        kern, loc = timed(lambda: depth_correlation_local_loss_step(d, p, 0.05, P, (5, 3)), "k_dlocal")
        K = ((H - 5) // P) * ((W - 3) // P)
        verdict = ""
        if (H, W) == (1080, 1920) and P in (16, 32, 64):
            verdict = "   bar 1.5: " + ("met" if loc <= 1.5 * glob else f"MISSED by {loc / glob - 1.5:.2f}")
        say(f"    local P={P:<3} K={K:<6}" + cols(kern) + f"   step {loc:7.2f}   {mb / loc:5.2f} TB/s   local / global {loc / glob:5.2f}{verdict}")


def smooth_rows(d, image, H, W, plane, rate, glob, bar=1.75):
    kw, once = timed(lambda: depth_edge_weights(image, 1.0), "k_dsmooth")
    say(f"    edge weights 5 planes  " + cols(kw) + f"   call {once:7.2f}   (once per camera; {8.0 * H * W / 1e6:.1f} MB kept per camera)")
    w = depth_edge_weights(image, 1.0)
    buf = torch.zeros(1, H, W, device=dev)
    for acc, planes in ((0, {"k_dsmooth_stats": 3, "k_dsmooth_grad": 4}), (1, {"k_dsmooth_stats": 3, "k_dsmooth_grad": 5})):
        kern, step = timed(lambda: depth_smoothness_loss_step(d, w, 0.05, grad_out=buf if acc else None), "k_dsmooth")
        total = sum(planes.values())
        verdict = ""
        if (H, W) == (1080, 1920) and acc == 0:
            verdict = f"   bar {bar}: " + ("met" if step <= bar * glob else f"MISSED by {step / glob - bar:.2f}")
        say(f"    smoothness acc={acc} {total} planes  " + cols(kern, lambda k: f" (bytes alone {planes.get(k, 0) * plane / rate:5.2f})") +
            f"   step {step:7.2f}   {total * plane / step:5.2f} TB/s   smoothness / correlation {step / glob:5.2f}{verdict}")


say(f"== 1. the step entries, us (kernel trace per launch; stream time per call over {REPS} back-to-back calls)")
for H, W in ((1080, 1920), (576, 1024)):
    g = torch.Generator().manual_seed(0)
    d = (20.0 + torch.rand(1, H, W, generator=g)).to(dev)
    p = (1.0 / d[0] + 0.01 * torch.rand(H, W, generator=g).to(dev)).contiguous()
    image = torch.rand(3, H, W, generator=g).to(dev)
    plane = 4.0 * H * W / 1e6                                       # MB
    kern, glob = timed(lambda: depth_correlation_loss_step(d, p, 0.05), "k_dcorr")
    if args.term == "smooth":
        src, dst = torch.rand(4, H, W, device=dev), torch.empty(4, H, W, device=dev)
        _, copy = timed(lambda: dst.copy_(src), "k_none")
        rate = 8 * plane / copy                                     # TB/s of a plain copy at this size
        say(f"  {W}x{H}  (one plane {plane:.1f} MB; a device copy of 4 planes takes {copy:.2f} us: {rate:.2f} TB/s)")
        say(f"    correlation  5 planes  " + cols(kern) + f"   step {glob:7.2f}   {5 * plane / glob:5.2f} TB/s")
        smooth_rows(d, image, H, W, plane, rate, glob)
    else:
        say(f"  {W}x{H}  ({5 * plane:.1f} MB moved per step)")
        say(f"    global            " + cols(kern) + f"   step {glob:7.2f}   {5 * plane / glob:5.2f} TB/s")
        if args.term == "local":
            local_rows(d, p, H, W, 5 * plane, glob)

if args.iters > 0:                                              # (--iters 0: the step entries alone)
    say(f"== 2. GSTrainer.training(), 200 000 Gaussians, 1920x1080, iterations / s over {args.iters} iterations, off / on interleaved")
    N, H, W = 200_000, 1080, 1920
    with tempfile.TemporaryDirectory() as tmp:
        tr = measure.synthetic_scene(dev, N, H, W, 2, args.iters + 1, tmp)        # (+ 1: no checkpoint inside a timed window)
        if needs_prior:
            from syn3r_amd.gs import GaussianModel, GSTrainer
            from syn3r_amd.launch import truth_disparity
            from syn3r_amd.synthetic import synthetic_gaussians
            m, s, q, o, sh = synthetic_gaussians(N, seed=0)
            logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
            truth = GSTrainer(GaussianModel(m, torch.log(s), q, logit, sh, device=dev), [])
            for cam in tr.scene.getTrainCameras():
                cam.depth_image = truth_disparity(truth, cam)
            del truth
        if args.term == "local":
            tr.opt.depth_patch_size = 32
        rates = {0.0: [], 0.05: []}
        for weight in (0.0, 0.05, 0.0, 0.05, 0.0, 0.05):        # interleaved: box drift shows as a spread, not as a bias
            setattr(tr.opt, option, weight)
            tr.training(0, iterations=50, disable_densification=True)      # warm-up: capacities, workspaces, the cameras' edge weights
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.training(0, iterations=args.iters, disable_densification=True)
            torch.cuda.synchronize()
            rates[weight].append(args.iters / (time.perf_counter() - t0))
    for k, (a, b) in enumerate(zip(rates[0.0], rates[0.05])):
        say(f"  round {k}: off {a:.1f} /s   on {b:.1f} /s   on/off {b / a:.4f}   (+{(1 / b - 1 / a) * 1e6:.1f} us per step)")
if out is not None:
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text("\n".join(lines) + "\n")
