"""Cost of FSGS' proximity-guided Gaussian unpooling (csrc/knn.hip): device time of syn3r_knn3_graph against syn3r_knn3_mean_dist2
(the yardstick: same boxes, same pruning) alternating in one process, and of the count + emit pair at the 0.8-quantile score
threshold, at 10 000 / 200 000 / 1 000 000 points of a clustered cloud and of synthetic_gaussians; what share of the launcher's
synthetic scene the trainer's default factors select at its first densification; GSTrainer.training() iterations / s at 200 000
Gaussians / 1080p, densifying every 100 iterations, with the unpooling off and on (developer tool).
usage: python tools/unpool_bench.py [trainer iterations per run, 0 = skip the trainer part]"""
import json
import math
import sys
import tempfile
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
import _devlib  # noqa: F401  (SYN3R_LIB_OVERRIDE=<other build>: explicit, tool-side)
from syn3r_amd import _lib as L
from syn3r_amd import launch, measure
from syn3r_amd.gs.train_ops import knn3_graph, knn3_mean_dist2, proximity_unpool
from syn3r_amd.synthetic import synthetic_gaussians

its = int(sys.argv[1]) if len(sys.argv) > 1 else 400
dev = torch.device("cuda", 0)
res = {}


def clustered(n: int, seed: int = 7) -> np.ndarray:          # dense blobs + sparse background (the k-d tree test's cloud)
    g = np.random.default_rng(seed)
    c = g.normal(size=(8, 3)).astype(np.float32) * 3
    p = c[g.integers(0, 8, n)] + g.normal(size=(n, 3)).astype(np.float32) * np.float32(0.05)
    p[: n // 20] = g.normal(size=(n // 20, 3)).astype(np.float32) * 20
    return p.astype(np.float32)


def event_ms(fn, reps: int) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


# ---- the two searches, alternating; then the selection + emission
for gen in ("clustered", "synthetic"):
    for n in (10_000, 200_000, 1_000_000):
        pts = (torch.from_numpy(clustered(n)) if gen == "clustered" else synthetic_gaussians(n, seed=0)[0]).to(dev).contiguous()
        reps, rounds = (50, 4) if n <= 200_000 else (10, 4)
        for _ in range(3):                                   # warm-up: code objects, workspaces
            knn3_mean_dist2(pts)
            knn3_graph(pts)
        torch.cuda.synchronize()
        mean_ms, graph_ms = [], []
        for r in range(rounds):                              # alternating order: drift shows as a spread, not as a bias
            for which in (("mean", "graph") if r % 2 == 0 else ("graph", "mean")):
                if which == "mean":
                    mean_ms.append(event_ms(lambda: knn3_mean_dist2(pts), reps))
                else:
                    graph_ms.append(event_ms(lambda: knn3_graph(pts), reps))
        with L.kernel_trace() as tr_:                        # the search kernels alone (HIP events on the dispatches)
            for _ in range(5):
                knn3_mean_dist2(pts)
                knn3_graph(pts)
            torch.cuda.synchronize()
        kern = {k: round(ms / c, 4) for k, (c, ms) in tr_.result.items() if k in ("k_knn3", "k_knn3_graph")}
        # count + emit at the 0.8 quantile of the cloud's own scores, scale test off (every fifth Gaussian is a source)
        dist2, index = knn3_graph(pts)
        score = ((dist2[:, 0] + dist2[:, 1]) + dist2[:, 2]) / 3.0
        st = float(score.cpu().double().quantile(0.8)) if n <= 200_000 else float(np.quantile(score.cpu().numpy(), 0.8))
        g = torch.Generator().manual_seed(1)
        ls = torch.log(0.002 + 0.048 * torch.rand(n, 3, generator=g)).to(dev)
        op, conf = torch.randn(n, generator=g).to(dev), torch.rand(n, generator=g).to(dev)
        lib = L.load()
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.syn3r_gaussian_unpool_workspace_bytes(n), dtype=torch.uint8, device=dev)
        sp = L.stream_ptr(dev)
        do_count = lambda: L.check(lib.syn3r_gaussian_unpool_count(L.ptr(dist2), L.ptr(ls), n, st, -math.inf, L.ptr(count), L.ptr(ws),
                                                                   ws.numel(), sp), "count")
        do_count()
        S = int(count.item())
        M = 3 * S
        outs = [torch.empty(s, device=dev) for s in ((M, 3), (M, 3), (M,), (M, 4), (M,))]
        do_emit = lambda: L.check(lib.syn3r_gaussian_unpool_emit(L.ptr(pts), L.ptr(ls), L.ptr(op), L.ptr(conf), L.ptr(index), n, S, M,
                                                                 *[L.ptr(t) for t in outs], L.ptr(ws), ws.numel(), sp), "emit")
        do_emit()
        pair_ms = event_ms(lambda: (do_count(), do_emit()), 50)
        t0 = time.perf_counter()
        for _ in range(5):
            proximity_unpool(pts, ls, op, conf, st, -math.inf)
        torch.cuda.synchronize()
        res[f"{gen}_{n}"] = {"mean_dist2_ms": [round(v, 4) for v in mean_ms], "graph_ms": [round(v, 4) for v in graph_ms],
                             "graph_over_mean": round(float(np.median(graph_ms) / np.median(mean_ms)), 3), "search_kernel_ms": kern,
                             "sources": S, "count_emit_ms": round(pair_ms, 4),
                             "proximity_unpool_wall_ms": round(1000.0 * (time.perf_counter() - t0) / 5, 3)}
        print(json.dumps({f"{gen}_{n}": res[f"{gen}_{n}"]}), flush=True)

# ---- what the trainer's default factors select on the launcher's synthetic scene at its first densification
with tempfile.TemporaryDirectory() as tmp:
    args = launch.parse(["--scenes", "synthetic:0", "--iterations", "600", "--model_path", tmp, "--use_proximity_densify", "1"])
    tr = launch.synthetic_scene("synthetic:0", args, dev)["trainer"]
    tr.opt.use_proximity_densify = True
    seen = []
    orig = tr.proximity_unpool

    def recorded(extent):
        g = tr.gaussians
        d2, _ = knn3_graph(g._xyz.detach())
        score = (((d2[:, 0] + d2[:, 1]) + d2[:, 2]) / 3.0).cpu().double()
        scale = g.get_scaling.detach().max(dim=1).values.cpu().double()
        m = orig(extent)
        seen.append({"iteration": tr.iteration + 1, "gaussians": int(score.shape[0]), "extent": round(extent, 4),
                     "score_thresh": tr.opt.proximity_dist_factor * extent, "scale_thresh": tr.opt.proximity_scale_factor * extent,
                     "score_quantiles_50_80_99_max": [float(score.quantile(q)) for q in (0.5, 0.8, 0.99, 1.0)],
                     "scale_quantiles_50_99_max": [float(scale.quantile(q)) for q in (0.5, 0.99, 1.0)],
                     "sources": m // 3, "share": (m // 3) / score.shape[0]})
        return m
    tr.proximity_unpool = recorded
    tr.training(0, iterations=600)
    res["default_factors_on_launcher_scene"] = seen[0] if seen else None
    print(json.dumps({"default_factors_on_launcher_scene": res["default_factors_on_launcher_scene"]}), flush=True)

# ---- the trainer with the unpooling off / on: N stays 200 000 (no clone / split / prune fires, the unpooling finds no source), so
# the runs differ by the operator alone - graph + count + the host read - once per 100 iterations (the emit launch is timed above)
if its > 0:
    N, H, W = 200_000, 1080, 1920
    with tempfile.TemporaryDirectory() as tmp:
        tr = measure.synthetic_scene(dev, N, H, W, 2, its, tmp)
        tr.scene.model_path = None                           # no checkpoint writes inside the timed runs
        o = tr.opt
        o.densify_from_iter, o.densification_interval, o.densify_grad_threshold, o.prune_min_opacity = 50, 100, 1e9, 0.0
        o.opacity_reset_interval, o.proximity_until_iter, o.proximity_dist_factor = 10**9, 10**9, 1e9
        calls = []
        orig = tr.proximity_unpool
        tr.proximity_unpool = lambda e: calls.append(1) or orig(e)
        for flag in (False, True, False, True, False, True):  # interleaved: box drift shows as a spread, not as a bias
            o.use_proximity_densify = flag
            tr.training(0, iterations=50, disable_densification=True)      # warm-up: capacities, workspaces
            torch.cuda.synchronize()
            calls.clear()
            t0 = time.perf_counter()
            tr.training(0, iterations=its)
            torch.cuda.synchronize()
            res.setdefault(f"trainer_it_s_unpool_{'on' if flag else 'off'}", []).append(round(its / (time.perf_counter() - t0), 1))
            res[f"trainer_unpool_calls_{'on' if flag else 'off'}"] = len(calls)
        res["trainer_gaussians_at_end"] = int(tr.gaussians._xyz.shape[0])
print(json.dumps(res))
