"""What 3DGS-MCMC (`OptimizationParams.mcmc`: csrc/mcmc.hip) costs on the bench scene (developer tool; profiles/r16/mcmc.txt).

    python tools/mcmc_cost.py [--iters 200] [--rounds 3] [--out profiles/r16/mcmc.txt]

    1. the kernels per launch at the bench scene's Gaussian count (200 000): the library's own kernel trace (event timestamps on the
       dispatch packets), 50 calls after 10.  For the noise and the regulariser pass, the two that run every step, the bytes each
       moves, the rate that makes and the time those bytes alone allow at the achievable HBM rate (6.3 TB/s) - at 200 000 Gaussians
       both working sets sit in the caches from the step before, so the floor is a bound from below, not a prediction
    2. the trainer's explicit step (GSTrainer.train_step: raw-parameter render, fused photometric loss, backward, fused Adam; density
       control off, so the option adds the regulariser's two launches and the noise launch) with the option off / on, alternating:
       iterations per second at the bench scene's image size"""
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
ap.add_argument("--out", type=str, default=str(Path(__file__).resolve().parents[1] / "profiles" / "r16" / "mcmc.txt"))
mine = ap.parse_args()
sys.argv = sys.argv[:1]
args = bench.parse()

from syn3r_amd import _lib as L  # noqa: E402
from syn3r_amd import raster  # noqa: E402
from syn3r_amd import synthetic  # noqa: E402
from syn3r_amd.gs import Camera, GaussianModel, GSTrainer, OptimizationParams  # noqa: E402
from syn3r_amd.gs import mcmc as M  # noqa: E402
from syn3r_amd.gs import train_ops as T  # noqa: E402

HBM = 6.3e12                              # achievable bytes / s of the MI355X
lines = []


def say(text: str):
    print(text, flush=True)
    lines.append(text)


dev = torch.device("cuda", 0)
loop = bench.RasterLoop(args, dev)
H, W, N = args.height, args.width, args.gaussians
say(f"scene: {N} Gaussians, {H}x{W}; {mine.iters} iterations per timing, {mine.rounds} rounds, off / on alternating")

say("== 1. mcmc kernels, us per launch (kernel trace, 50 calls)")
g_m, g_s, g_q, g_o, g_sh = synthetic.synthetic_gaussians(N, seed=args.seed)
# a fifth of the Gaussians dead, so that the sampler and the relocation have work every call
g_o = torch.where(torch.arange(N) % 5 == 0, torch.full_like(g_o, 1e-3), g_o)
logit0 = torch.log(g_o.clamp(1e-3, 1 - 1e-3) / (1 - g_o.clamp(1e-3, 1 - 1e-3)))
xyz, ls, rot, feat = g_m.to(dev), torch.log(g_s).to(dev), g_q.to(dev).contiguous(), g_sh.to(dev).contiguous()
grad_o, grad_s = torch.zeros(N, device=dev), torch.zeros(N, 3, device=dev)
row = int(feat[0].numel())
dead, clamp = M.dead_logit(0.005), M.clamp_opacity(0.005)


def once(step):
    logit = logit0.to(dev)                # (the relocation revives the dead: start every call from the same state)
    T.mcmc_noise(xyz, ls, rot, logit, 80.0, 0, step)
    T.mcmc_reg_step(logit, ls, 0.01, 0.01, grad_o, grad_s)
    w = T.mcmc_weights(logit, dead)
    src, counts = T.mcmc_sample(w, N // 20, 0, step)
    T.mcmc_relocate(src, counts, xyz, feat, logit, ls, rot, [None] * 10, clamp)


for k in range(10):
    once(k + 1)
torch.cuda.synchronize()
with L.kernel_trace(only="k_mcmc") as tr:
    for k in range(50):
        once(k + 11)
    torch.cuda.synchronize()
# noise: reads xyz 12, log-scales 12, rotation 16, logit 4, writes xyz 12; regulariser pass: reads logit 4, log-scales 12 and the two
# gradients 16, writes the gradients 16
moved = {"k_mcmc_noise": 56 * N, "k_mcmc_reg_pass": 48 * N}
for name, (calls, ms) in sorted(tr.result.items()):
    us = ms / calls * 1e3
    rate = ""
    if name in moved:
        rate = (f"   {moved[name] / 1e6:6.1f} MB   {moved[name] / (us * 1e-6) / 1e12:5.2f} TB/s   bytes alone at 6.3 TB/s: "
                f"{moved[name] / HBM * 1e6:5.2f} us")
    say(f"  {name:<22} calls {calls:4d}   avg {us:8.2f} us{rate}")

say("== 2. trainer explicit step (0.8 L1 + 0.2 (1 - SSIM), fused Adam; density control off), iterations per second")
fx = W / (2 * np.tan(np.deg2rad(60.0) / 2))
K = np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], dtype=np.float32)
pose = np.eye(4, dtype=np.float32)
g_m, g_s, g_q, g_o, g_sh = synthetic.synthetic_gaussians(N, seed=args.seed)
logit = torch.log(g_o.clamp(1e-3, 1 - 1e-3) / (1 - g_o.clamp(1e-3, 1 - 1e-3)))
# FSGS's learning rates x 1e-3, as bench.RasterLoop.full_iteration_rate: the target is noise, the timing should be of a steady scene
# (the noise scale follows the position rate: 5e5 x 1.6e-7)
rates = dict(position_lr=1.6e-7, feature_lr=2.5e-6, opacity_lr=5e-5, scaling_lr=5e-6, rotation_lr=1e-6)
trainers, cams = {}, {}
for on in (False, True):
    gm = GaussianModel(g_m, torch.log(g_s), g_q, logit, g_sh, device=dev)
    cams[on] = Camera.from_w2c(pose, K, H, W, image=loop.target.cpu(), data_device=dev)
    trainers[on] = GSTrainer(gm, [cams[on]], OptimizationParams(mcmc=on, mcmc_cap_max=N, **rates))
raster.set_pair_count_mode("sync")
for on in (False, True):
    with torch.no_grad():
        trainers[on].render_view(cams[on])                # seeds the async pair capacity of the shape
raster.set_pair_count_mode("async")
for on in (False, True):
    for _ in range(10):
        trainers[on].train_step(cams[on])
torch.cuda.synchronize()
for r in range(mine.rounds):
    rates_ = []
    for on in (False, True):
        t0 = time.perf_counter()
        for _ in range(mine.iters):
            trainers[on].train_step(cams[on])
        torch.cuda.synchronize()
        rates_.append(mine.iters / (time.perf_counter() - t0))
    say(f"  round {r}: off {rates_[0]:.1f} /s   on {rates_[1]:.1f} /s   on/off {rates_[1] / rates_[0]:.4f}   "
        f"(+{(1 / rates_[1] - 1 / rates_[0]) * 1e6:.1f} us per step)")
raster.flush_pair_checks()
Path(mine.out).parent.mkdir(parents=True, exist_ok=True)
Path(mine.out).write_text("\n".join(lines) + "\n")
