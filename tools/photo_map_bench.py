"""Cost of the per-pixel weight map in the fused photometric loss (csrc/photo_loss.hip, `photometric_loss_step(weight_map=)`): device
time per kernel of the step with and without a map at 3x1080x1920 and 3x576x1024 (HIP events on the dispatches, the two variants
alternating, several rounds so that the run-to-run spread shows), and GSTrainer.training() iterations / s at 200 000 Gaussians /
1080p with a map on every camera and without (developer tool).
usage: python tools/photo_map_bench.py [iterations]
       python tools/photo_map_bench.py --digest     sha256 of what the entries WITHOUT a map leave on seeded 1080p inputs: run it on
                                                    two builds (SYN3R_LIB_OVERRIDE=<other build>) and compare the lines"""
import hashlib
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
from syn3r_amd.gs.train_ops import l1_loss, l1_loss_step, photometric_loss, photometric_loss_step

dev = torch.device("cuda", 0)


def inputs(H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(3, H, W, generator=g)
    b = (a + 0.2 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    m = torch.rand(H, W, generator=g)
    return a.to(dev), b.to(dev), m.to(dev)


if "--digest" in sys.argv:
    sha = lambda *ts: hashlib.sha256(b"".join(t.detach().cpu().contiguous().numpy().tobytes() for t in ts)).hexdigest()[:16]
    out = {}
    for H, W in ((1080, 1920), (1080, 1918)):            # the 16-byte row runs and the scalar ones
        a, b, _ = inputs(H, W)
        go = torch.tensor(1.5, device=dev)
        for lam in (0.2, 1.0):
            x = a.clone().requires_grad_(True)
            loss, parts = photometric_loss(x, b, lam, 0.7, return_parts=True)
            (loss * 1.5).backward()
            l2, p2, g2 = photometric_loss_step(a, b, lam, 0.7, grad_loss=go)
            out[f"photo_{W}x{H}_lam{lam}"] = [sha(loss, parts, x.grad), sha(l2, p2, g2)]
        x = a.clone().requires_grad_(True)
        loss = l1_loss(x, b, 0.7)
        (loss * 1.5).backward()
        l2, g2 = l1_loss_step(a, b, 0.7, grad_loss=go)
        out[f"l1_{W}x{H}"] = [sha(loss, x.grad), sha(l2, g2)]
    print(json.dumps({"library": str(L.lib_path()), "digests": out}))
    sys.exit(0)

its = int(sys.argv[1]) if len(sys.argv) > 1 else 300
res = {}

# ---- the step entry alone, per kernel; variants alternate inside a round
for H, W in ((1080, 1920), (576, 1024)):
    a, b, m = inputs(H, W)
    variants = {"plain": None, "map": m}
    for _ in range(20):
        for wm in variants.values():
            photometric_loss_step(a, b, 0.2, 0.7, weight_map=wm)
    torch.cuda.synchronize()
    reps, rounds = 100, 5
    per = {k: [] for k in variants}
    stream = {k: [] for k in variants}
    for _ in range(rounds):
        for name, wm in variants.items():
            with L.kernel_trace() as tr_:
                for _ in range(reps):
                    photometric_loss_step(a, b, 0.2, 0.7, weight_map=wm)
                torch.cuda.synchronize()
            per[name].append({k: round(1000.0 * ms / c, 2) for k, (c, ms) in tr_.result.items() if "k_photo" in k})
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                photometric_loss_step(a, b, 0.2, 0.7, weight_map=wm)
            e1.record()
            torch.cuda.synchronize()
            stream[name].append(round(1000.0 * e0.elapsed_time(e1) / reps, 2))
    entry = {}
    for name in variants:
        kernels = sorted(per[name][0])
        entry[name] = {"kernels_us_per_round": {k: [r[k] for r in per[name]] for k in kernels},
                       "kernels_us_median": {k: sorted(r[k] for r in per[name])[rounds // 2] for k in kernels},
                       "stream_us_per_call_per_round": stream[name]}
    res[f"step_{W}x{H}"] = entry

# ---- the trainer without / with a map on every camera
N, H, W = 200_000, 1080, 1920
with tempfile.TemporaryDirectory() as tmp:
    tr = measure.synthetic_scene(dev, N, H, W, 2, its, tmp)
    g = torch.Generator().manual_seed(3)
    maps = [torch.rand(H, W, generator=g) for _ in tr.scene.getTrainCameras()]
    for on in (False, True, False, True):              # interleaved: box drift shows as a spread, not as a bias
        for cam, m in zip(tr.scene.getTrainCameras(), maps):
            cam.confidence_map = m if on else None
        tr.training(0, iterations=50, disable_densification=True)      # warm-up: capacities, workspaces
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.training(0, iterations=its, disable_densification=True)
        torch.cuda.synchronize()
        res.setdefault("trainer_it_s_" + ("map" if on else "plain"), []).append(round(its / (time.perf_counter() - t0), 1))
print(json.dumps(res))
