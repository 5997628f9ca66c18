"""Cost of FSGS' depth-correlation term (csrc/depth_loss.hip): device time of syn3r_depth_corr_loss_step per call at 1920x1080
and 1024x576 (per kernel, HIP events on the dispatches), and GSTrainer.training() iterations / s at 200 000 Gaussians / 1080p with
the term off and on (developer tool; the priors are the truth cloud's disparities).
usage: python tools/depth_loss_bench.py [iterations]"""
import json
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
from syn3r_amd.gs.train_ops import depth_correlation_loss_step
from syn3r_amd.launch import truth_disparity
from syn3r_amd.synthetic import synthetic_gaussians

its = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
dev = torch.device("cuda", 0)
res = {}

# ---- the step entry alone
for H, W in ((1080, 1920), (576, 1024)):
    g = torch.Generator().manual_seed(0)
    d = (20.0 + torch.rand(1, H, W, generator=g)).to(dev)
    p = (1.0 / d[0] + 0.01 * torch.rand(H, W, generator=g).to(dev)).contiguous()
    for _ in range(20):
        depth_correlation_loss_step(d, p, 0.05)
    torch.cuda.synchronize()
    reps = 200
    with L.kernel_trace() as tr_:
        for _ in range(reps):
            depth_correlation_loss_step(d, p, 0.05)
        torch.cuda.synchronize()
    kern = {k: round(1000.0 * ms / c, 2) for k, (c, ms) in tr_.result.items() if "dcorr" in k}
    # back-to-back calls: the device time per step including the gap between its two launches
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        depth_correlation_loss_step(d, p, 0.05)
    e1.record()
    torch.cuda.synchronize()
    res[f"step_{W}x{H}"] = {"kernels_us": kern, "kernels_sum_us": round(sum(kern.values()), 2),
                            "stream_us_per_call": round(1000.0 * e0.elapsed_time(e1) / reps, 2)}

# ---- the trainer with the term off / on
N, H, W = 200_000, 1080, 1920
m, s, q, o, sh = synthetic_gaussians(N, seed=0)
logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
truth = GSTrainer(GaussianModel(m, torch.log(s), q, logit, sh, device=dev), [])
with tempfile.TemporaryDirectory() as tmp:
    tr = measure.synthetic_scene(dev, N, H, W, 2, its, tmp)
    for cam in tr.scene.getTrainCameras():
        cam.depth_image = truth_disparity(truth, cam)
    del truth
    for dw in (0.0, 0.05, 0.0, 0.05):                  # interleaved: box drift shows as a spread, not as a bias
        tr.opt.depth_weight = dw
        tr.training(0, iterations=50, disable_densification=True)      # warm-up: capacities, workspaces
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.training(0, iterations=its, disable_densification=True)
        torch.cuda.synchronize()
        res.setdefault(f"trainer_it_s_depth_weight_{dw}", []).append(round(its / (time.perf_counter() - t0), 1))
print(json.dumps(res))
