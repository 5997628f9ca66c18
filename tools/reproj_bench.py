"""Cost and outcome of the trainer's multi-view photometric reprojection term (developer tool; csrc/reproj.hip: k_reproj_*).

    python tools/reproj_bench.py [--iters 300 | --iters 0] [--outcome] [--out FILE]

    1. syn3r_photo_reproj_loss_step at 1920x1080 for S = 1, 2, 4 sources: per kernel (the library's kernel trace: event timestamps on
       the dispatch packets) and per step (device events around 200 back-to-back calls), and in the same run
       syn3r_depth_smooth_loss_step, a device copy of the same byte count, and the launch floor (a one-block elementwise launch).
       Algorithmic bytes of a step: the statistics pass reads D, a and the 3 target planes, gathers each source's 3 planes once and
       writes 2 planes; the gradient pass reads 3 planes and writes 2: 12 + 3 S planes.  The bar: the step takes at most
       2 x (bytes / the copy's rate + two launch floors) - the factor the existing depth terms reached against the copy.
    2. The step on the RENDERED depth and alpha of a 200 000-Gaussian scene at 1080p (five input views; S = 1, 2, 4 nearest as
       sources), then GSTrainer.training() iterations / s on that scene (S = 2), term off and on, interleaved.  --iters 0: skipped.
    3. --outcome: the 72 x 128 three-camera synthetic scene, 300 iterations without densification, for reproj_weight in
       {0, 0.05, 0.1, 0.2, 0.5, 1, 2}: photometric loss, mean absolute error of the alpha-normalised rendered depth against the truth
       cloud's, held-out PSNR.  The weight to quote: the largest whose photometric loss stays within 1.5 x the off run's.
    --out defaults to profiles/r22/reproj.txt."""
import argparse
import sys
import tempfile
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
import _devlib  # noqa: F401  (SYN3R_LIB_OVERRIDE=<other build>: explicit, tool-side)
from syn3r_amd import _lib as L
from syn3r_amd import measure
from syn3r_amd.gs import reproj as reproj_host
from syn3r_amd.gs.train_ops import depth_edge_weights, depth_smoothness_loss_step, photo_reprojection_loss_step

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=300)
ap.add_argument("--outcome", action="store_true")
ap.add_argument("--out", type=str, default=None)
args = ap.parse_args()
out = Path(args.out or Path(__file__).resolve().parents[1] / "profiles" / "r22" / "reproj.txt")
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


def cols(kern):
    return "  ".join(f"{k} {v:7.2f}" for k, v in kern.items())


def views_for(H, W, S):
    """S sources on an x / y baseline around the target: about a tenth of the image of parallax at depth 3"""
    f = W / (2 * np.tan(np.radians(30)))
    k = np.array([f, f, (W - 1) / 2, (H - 1) / 2])
    table = np.zeros((S, 16))
    for s, (bx, by) in enumerate([(0.3, 0.0), (-0.3, 0.0), (0.0, 0.2), (0.0, -0.2)][:S]):
        table[s] = np.concatenate([np.eye(3).reshape(9), [bx, by, 0.0], k])
    return reproj_host.ReprojViews(k.astype(np.float32), table.astype(np.float32))


say(f"== 1. the step entry, us (kernel trace per launch; stream time per call over {REPS} back-to-back calls)")
H, W = 1080, 1920
g = torch.Generator().manual_seed(0)
plane = 4.0 * H * W / 1e6                                           # MB
ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32) / H, torch.arange(W, dtype=torch.float32) / W, indexing="ij")
alpha = (0.6 + 0.4 * torch.rand(1, H, W, generator=g)).to(dev)
# a SMOOTH surface, as a render's: neighbouring pixels map to neighbouring source positions (noise in the depth would scatter the taps)
depth = ((3.0 + 0.5 * torch.sin(6.0 * xs + 4.0 * ys))[None].to(dev) * alpha).contiguous()
images = [torch.rand(3, H, W, generator=g).to(dev) for _ in range(5)]
tiny = torch.zeros(256, device=dev)
_, floor = timed(lambda: tiny.add_(0.0), "k_none")
say(f"  {W}x{H}  (one plane {plane:.1f} MB; launch floor, a one-block elementwise launch on the stream: {floor:.2f} us)")
w = depth_edge_weights(images[0], 1.0)
kern, smooth = timed(lambda: depth_smoothness_loss_step(depth, w, 0.05), "k_dsmooth")
say(f"    smoothness  7 planes  " + cols(kern) + f"   step {smooth:7.2f}   {7 * plane / smooth:5.2f} TB/s")
for S in (1, 2, 4):
    planes = 12 + 3 * S
    half = (planes + 1) // 2
    src, dst = torch.rand(half, H, W, device=dev), torch.empty(half, H, W, device=dev)
    _, copy = timed(lambda: dst.copy_(src), "k_none")
    rate = 2 * half * plane / copy                                  # TB/s of a plain copy that moves (about) the step's bytes
    del src, dst
    v = views_for(H, W, S)
    kern, step = timed(lambda: photo_reprojection_loss_step(depth, alpha, images[0], images[1:1 + S], v, 0.1, 0.5), "k_reproj")
    bar = 2.0 * (planes * plane / rate + 2 * floor)
    say(f"    reprojection S={S} {planes} planes  " + cols(kern) + f"   step {step:7.2f}   {planes * plane / step:5.2f} TB/s   copy of "
        f"{2 * half} planes {copy:6.2f} us ({rate:.2f} TB/s)   bar {bar:6.2f}: " + ("met" if step <= bar else f"MISSED by {step - bar:.2f} us")
        + f"   reprojection / smoothness {step / smooth:5.2f}")
buf_d, buf_a = torch.zeros(1, H, W, device=dev), torch.zeros(1, H, W, device=dev)
kern, step = timed(lambda: photo_reprojection_loss_step(depth, alpha, images[0], images[1:3], views_for(H, W, 2), 0.1, 0.5, grad_out=buf_d,
                                                        grad_alpha_out=buf_a), "k_reproj")
say(f"    reprojection S=2, both gradients ADDED (20 planes)  " + cols(kern) + f"   step {step:7.2f}")
del images, depth, alpha, w, buf_d, buf_a

if args.iters > 0:
    say(f"== 2. GSTrainer.training(), 200 000 Gaussians, 1920x1080, 5 input views (S = 2: reproj_sources), iterations / s over {args.iters} iterations, "
        "off / on interleaved")
    with tempfile.TemporaryDirectory() as tmp:
        tr = measure.synthetic_scene(dev, 200_000, H, W, 5, args.iters + 1, tmp)
        # the step on an actual RENDER (depth discontinuities at silhouettes, alpha below alpha_min in places): the middle camera's
        # depth and alpha, its 1, 2, 4 nearest input views as sources
        cams = tr.scene.getTrainCameras()
        with torch.no_grad():
            o = tr.render_view(cams[2])
        rd, ra = o["depth"].detach().contiguous(), o["alpha"].detach().contiguous()
        for S in (1, 2, 4):
            imgs, v, _ = tr.reproj.get(cams[2], cams, S, 45.0)
            kern, step = timed(lambda: photo_reprojection_loss_step(rd, ra, cams[2].original_image, imgs, v, 0.1, 0.5), "k_reproj")
            say(f"  rendered depth of the scene, S={S}  " + cols(kern) + f"   step {step:7.2f}")
        del o, rd, ra
        rates = {0.0: [], 0.1: []}
        for weight in (0.0, 0.1, 0.0, 0.1, 0.0, 0.1):               # interleaved: box drift shows as a spread, not as a bias
            tr.opt.reproj_weight = weight
            tr.training(0, iterations=30, disable_densification=True)          # warm-up: capacities, workspaces, the source cache
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.training(0, iterations=args.iters, disable_densification=True)
            torch.cuda.synchronize()
            rates[weight].append(args.iters / (time.perf_counter() - t0))
        del tr
    for k, (a, b) in enumerate(zip(rates[0.0], rates[0.1])):
        say(f"  round {k}: off {a:.1f} /s   on {b:.1f} /s   on/off {b / a:.4f}   (+{(1 / b - 1 / a) * 1e6:.1f} us per step)")

if args.outcome:
    from syn3r_amd import launch
    say("== 3. outcome: synthetic:0 (72 x 128, three input views, two held-out), 300 iterations, no densification")

    def depth_mae(tr, cams):
        """mean |alpha-normalised rendered depth - true depth| where the truth cloud is seen (`depth_image`: its disparity, 0 elsewhere)"""
        errs = []
        with torch.no_grad():
            for c in cams:
                o = tr.render_view(c)
                ok = (c.depth_image > 0) & (o["alpha"][0] >= 0.5)
                errs.append(float((o["depth"][0][ok] / o["alpha"][0][ok] - 1.0 / c.depth_image[ok]).abs().mean()))
        return float(np.mean(errs))

    def term_value(tr, cams):
        """mean e of the term (weight 1) over the input views, and the share of live pixels"""
        from syn3r_amd.gs.train_ops import photo_reprojection_loss
        vals = []
        with torch.no_grad():
            for c in cams:
                o = tr.render_view(c)
                images, views, _ = tr.reproj.get(c, cams, 2, 45.0)
                vals.append(photo_reprojection_loss(o["depth"], o["alpha"], c.original_image, images, views, 1.0, 0.5, return_parts=True)[1])
        p = torch.stack(vals).mean(0)
        return float(p[1]), float(p[2])

    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        for weight in (0.0, 0.05, 0.1, 0.2, 0.5, 1.0, 2.0):
            a = launch.parse(["--scenes", "synthetic:0", "--model_path", f"{tmp}/w{weight}", "--iterations", "300"])
            sc = launch.synthetic_scene("synthetic:0", a, dev)
            tr = sc["trainer"]
            cams = tr.scene.getTrainCameras()
            start, e_start = depth_mae(tr, cams), term_value(tr, cams)
            tr.opt.reproj_weight = weight
            tr.training(iterations=300, disable_densification=True)
            with torch.no_grad():
                photo = float(np.mean([float(tr._photo_loss(tr.render_view(c)["render"], c, False)[0]) for c in cams]))
            rows[weight] = (photo, start, depth_mae(tr, cams), tr.evaluate(sc["test_cameras"])["psnr"], tr.evaluate()["psnr"], e_start,
                            term_value(tr, cams))
    off = rows[0.0][0]
    for weight, (photo, start, mae, psnr, psnr_train, e0, e1) in rows.items():
        say(f"  reproj_weight {weight:<4}: photometric loss {photo:.5f} ({photo / off:4.2f} x off)   depth MAE {start:.5f} -> {mae:.5f}   "
            f"held-out PSNR {psnr:.3f}   training PSNR {psnr_train:.3f}   mean e {e0[0]:.5f} -> {e1[0]:.5f} (live {e1[1]:.3f})")
    ok = [wt for wt, r in rows.items() if wt > 0 and r[0] <= 1.5 * off]
    say(f"  largest weight whose photometric loss stays within 1.5 x the off run's: {max(ok) if ok else 'none'}")

out.parent.mkdir(parents=True, exist_ok=True)
out.write_text("\n".join(lines) + "\n")
