"""FSGS' proximity-guided Gaussian unpooling on the GPU (csrc/knn.hip: syn3r_knn3_graph, syn3r_gaussian_unpool_count / _emit;
train_ops.knn3_graph / proximity_unpool; GSTrainer.proximity_unpool inside densify_and_prune) against numpy restatements kept in
this file: a brute-force 3-NN graph in the kernel's fp32 operation order with the (d2, index) order, scipy's k-d tree as an
independent algorithm, and the selection / emission rule as stated in include/syn3r_hip.h."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32
CLOUDS = [("uniform", 4), ("uniform", 5), ("uniform", 1000), ("uniform", 1024), ("uniform", 1025), ("clustered", 6000),
          ("duplicates", 5000), ("planar", 3000), ("uniform", 20000)]
UNPOOL_CLOUDS = [("uniform", 1025), ("clustered", 6000), ("duplicates", 5000), ("planar", 3000), ("uniform", 20000)]


def _cloud(kind: str, n: int, seed: int) -> np.ndarray:
    """The generator of tests/test_knn_gpu.py (restated: that file is not imported)."""
    g = np.random.default_rng(seed)
    if kind == "uniform":
        return g.random((n, 3), dtype=np.float32) * np.float32(4.0) - np.float32(2.0)
    if kind == "clustered":
        c = g.normal(size=(8, 3)).astype(np.float32) * 3
        p = c[g.integers(0, 8, n)] + g.normal(size=(n, 3)).astype(np.float32) * np.float32(0.05)
        p[: n // 20] = g.normal(size=(n // 20, 3)).astype(np.float32) * 20
        return p.astype(np.float32)
    if kind == "duplicates":
        base = g.integers(0, 12, size=(n, 3)).astype(np.float32)
        base[: n // 4] = base[n // 4: n // 2][: n // 4]
        return base
    if kind == "planar":
        p = g.random((n, 3), dtype=np.float32)
        p[:, 2] = np.float32(0.5)
        return p
    raise ValueError(kind)


def graph_bruteforce(points: np.ndarray, chunk: int = 1024):
    """(dist2 [n,3] fp32, index [n,3] int32): d2 = (dx*dx + dy*dy) + dz*dz in fp32, the three smallest of every row under the
    order (d2, index).  Candidates = everything not above the third-smallest value (all ties included), taken in index order
    and sorted by d2 with a STABLE sort: equal distances keep the index order."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    n = p.shape[0]
    dist = np.empty((n, 3), dtype=np.float32)
    idx = np.empty((n, 3), dtype=np.int32)
    for s in range(0, n, chunk):
        q = p[s:s + chunk]
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[np.arange(q.shape[0]), np.arange(s, s + q.shape[0])] = np.inf
        third = np.partition(d2, 2, axis=1)[:, 2]
        for r in range(q.shape[0]):
            c = np.flatnonzero(d2[r] <= third[r])                       # ascending index
            o = np.argsort(d2[r, c], kind="stable")[:3]
            idx[s + r], dist[s + r] = c[o], d2[r, c[o]]
    return dist, idx


@functools.lru_cache(maxsize=None)
def _case(kind: str, n: int):
    p = _cloud(kind, n, seed=n)
    dist, idx = graph_bruteforce(p)
    return p, dist, idx


def _score(dist: np.ndarray) -> np.ndarray:
    return ((dist[:, 0] + dist[:, 1]) + dist[:, 2]) / F32(3.0)


def unpool_restated(xyz, log_s, op, conf, dist, idx, score_thresh, log_scale_thresh):
    """The rule of include/syn3r_hip.h in numpy, from a given graph: -> (dict of new rows, S, the two masks)."""
    by_score = _score(dist) > F32(score_thresh)
    by_scale = log_s.max(axis=1) > F32(log_scale_thresh)
    src = np.flatnonzero(by_score & by_scale)
    s3 = np.repeat(src, 3)
    dst = idx[src].reshape(-1)
    m = s3.shape[0]
    rot = np.zeros((m, 4), dtype=np.float32)
    rot[:, 0] = 1.0
    new = {"xyz": (xyz[s3] + xyz[dst]) * F32(0.5), "scaling": log_s[dst], "opacity": op[dst], "rotation": rot, "confidence": conf[dst]}
    return new, src.shape[0], by_score, by_scale


def _attrs(n: int):
    """log-scales log U(0.002, 0.05) per axis from default_rng(1), then opacity logits and confidences from the same stream."""
    g = np.random.default_rng(1)
    log_s = np.log(g.uniform(0.002, 0.05, size=(n, 3))).astype(np.float32)
    op = (g.normal(size=n) * 3).astype(np.float32)
    conf = g.uniform(0.1, 1.0, n).astype(np.float32)
    return log_s, op, conf


def _dev(gpu, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays]


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 4. graph, bit for bit
@pytest.mark.parametrize("kind,n", CLOUDS)
def test_graph_matches_bruteforce_bit_exact(kind, n, gpu):
    from syn3r_amd.gs.train_ops import knn3_graph, knn3_mean_dist2
    p, dist, idx = _case(kind, n)
    pts = torch.from_numpy(p).to(gpu)
    d_gpu, i_gpu = knn3_graph(pts)
    assert d_gpu.shape == (n, 3) and d_gpu.dtype == torch.float32 and i_gpu.shape == (n, 3) and i_gpu.dtype == torch.int32
    got_d, got_i = _np(d_gpu), _np(i_gpu)
    print(f"{kind} {n}: distance rows differing {int((got_d != dist).any(1).sum())}, index rows differing {int((got_i != idx).any(1).sum())}")
    assert np.array_equal(got_d, dist), (np.abs(got_d - dist).max(), int((got_d != dist).sum()))
    assert np.array_equal(got_i, idx), int((got_i != idx).any(1).sum())
    # ((d0 + d1) + d2) / 3 with an IEEE division (numpy; a device-side `/ 3.0` multiplies by the rounded reciprocal)
    assert torch.equal(torch.from_numpy(_score(got_d)), knn3_mean_dist2(pts).cpu())


def test_lattice_cloud_really_has_ties():
    """The (d2, index) order is exercised: most rows of the integer-lattice cloud have a tie inside their triple."""
    _, dist, _ = _case("duplicates", 5000)
    tied = int(((dist[:, 0] == dist[:, 1]) | (dist[:, 1] == dist[:, 2])).sum())
    print("rows with a tie inside the triple:", tied)
    assert tied > 2500


# ------------------------------------------------------------------------------------------------ 5. graph at 200 000 points
def test_graph_matches_kdtree_at_200k(gpu):
    from scipy.spatial import cKDTree
    from syn3r_amd.gs.train_ops import knn3_graph
    p = _cloud("clustered", 200_000, seed=7)
    d_gpu, i_gpu = knn3_graph(torch.from_numpy(p).to(gpu))
    got_d, got_i = _np(d_gpu).astype(np.float64), _np(i_gpu)
    p64 = p.astype(np.float64)
    d, i = cKDTree(p64).query(p64, k=5)
    assert np.array_equal(i[:, 0], np.arange(p.shape[0]))                # no duplicate points: the query point comes first
    assert np.allclose(got_d, d[:, 1:4] ** 2, rtol=2e-5, atol=1e-9), np.abs(got_d - d[:, 1:4] ** 2).max()
    near = d[:, 1:5]
    clear = ((near[:, 1:] - near[:, :-1]) > 1e-4 * near[:, 1:]).all(axis=1)      # the four nearest are separated
    left_out = int((~clear).sum())
    print(f"rows under the 1e-4 gap: {left_out} of {p.shape[0]}")
    assert left_out <= 0.005 * p.shape[0], left_out
    assert np.array_equal(got_i[clear], i[clear, 1:4].astype(np.int32)), int((got_i[clear] != i[clear, 1:4]).any(1).sum())


# ------------------------------------------------------------------------------------------------ 6. the operator
def _thresholds(dist):
    return float(F32(np.quantile(_score(dist), 0.8))), float(F32(math.log(0.02)))


@pytest.mark.parametrize("kind,n", UNPOOL_CLOUDS)
def test_unpool_matches_restatement(kind, n, gpu):
    from syn3r_amd.gs.train_ops import proximity_unpool
    p, dist, idx = _case(kind, n)
    log_s, op, conf = _attrs(n)
    st, lt = _thresholds(dist)
    exp, S, by_score, by_scale = unpool_restated(p, log_s, op, conf, dist, idx, st, lt)
    print(f"{kind} {n}: S = {S} ({S / n:.3f}), score alone {int(by_score.sum())}, scale alone {int(by_scale.sum())}")
    assert 0.05 <= S / n <= 0.5
    assert (by_score & ~by_scale).any() and (by_scale & ~by_score).any()          # neither test is vacuous
    got = proximity_unpool(*_dev(gpu, p, log_s, op, conf), st, lt)
    assert got["sources"] == S and got["count"] == 3 * S
    for k, e in exp.items():
        g = _np(got[k])
        assert g.shape == e.shape and g.dtype == np.float32, k
        assert np.array_equal(g, e), (k, int((g != e).sum()))


# ------------------------------------------------------------------------------------------------ 7. edges
def test_unpool_selects_nothing(gpu):
    from syn3r_amd.gs.train_ops import proximity_unpool
    p, dist, idx = _case("uniform", 1025)
    log_s, op, conf = _attrs(1025)
    for st, lt in ((float(_score(dist).max()), -math.inf), (-1.0, 0.0), (math.inf, -math.inf)):
        got = proximity_unpool(*_dev(gpu, p, log_s, op, conf), st, lt)
        assert got["count"] == 0 and got["sources"] == 0
        assert got["xyz"].shape == (0, 3) and got["rotation"].shape == (0, 4) and got["opacity"].shape == (0,)


@pytest.mark.parametrize("kind,n", [("uniform", 4), ("uniform", 1025), ("duplicates", 5000)])
def test_unpool_selects_everything(kind, n, gpu):
    """score_thresh = -1 and log_scale_thresh = -inf: every Gaussian is a source, M = 3 n (on the lattice cloud the midpoints
    of coincident points are the points themselves)."""
    from syn3r_amd.gs.train_ops import proximity_unpool
    p, dist, idx = _case(kind, n)
    log_s, op, conf = _attrs(n)
    exp, S, _, _ = unpool_restated(p, log_s, op, conf, dist, idx, -1.0, -math.inf)
    assert S == n
    got = proximity_unpool(*_dev(gpu, p, log_s, op, conf), -1.0, -math.inf)
    assert got["count"] == 3 * n
    for k, e in exp.items():
        assert np.array_equal(_np(got[k]), e), k
    if kind == "duplicates":
        coincident = dist.reshape(-1) == 0
        assert coincident.sum() > 1000 and np.array_equal(_np(got["xyz"])[coincident], np.repeat(p, 3, axis=0)[coincident])


def test_unpool_is_bitwise_repeatable(gpu):
    from syn3r_amd.gs.train_ops import proximity_unpool
    p, dist, _ = _case("clustered", 6000)
    log_s, op, conf = _attrs(6000)
    st, lt = _thresholds(dist)
    args = _dev(gpu, p, log_s, op, conf)
    a = proximity_unpool(*args, st, lt)
    a = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in a.items()}
    b = proximity_unpool(*args, st, lt)
    assert a["count"] == b["count"] > 0
    for k in ("xyz", "scaling", "opacity", "rotation", "confidence"):
        assert torch.equal(a[k], b[k]), k


def test_emit_refuses_a_buffer_one_row_short(gpu):
    """C-ABI: capacity 3 S - 1 is SYN3R_E_INVALID and the output buffers keep their contents; capacity 3 S then fills them."""
    from syn3r_amd import _lib as L
    from syn3r_amd.gs.train_ops import knn3_graph
    n = 1025
    p, dist, idx = _case("uniform", n)
    log_s, op, conf = _attrs(n)
    st, lt = _thresholds(dist)
    exp, S, _, _ = unpool_restated(p, log_s, op, conf, dist, idx, st, lt)
    pts, ls, o, c = _dev(gpu, p, log_s, op, conf)
    lib = L.load()
    d_gpu, i_gpu = knn3_graph(pts)
    count = torch.zeros(1, dtype=torch.int32, device=gpu)
    ws = torch.empty(lib.syn3r_gaussian_unpool_workspace_bytes(n), dtype=torch.uint8, device=gpu)
    L.check(lib.syn3r_gaussian_unpool_count(L.ptr(d_gpu), L.ptr(ls), n, st, lt, L.ptr(count), L.ptr(ws), ws.numel(), L.stream_ptr(gpu)),
            "count")
    assert int(count.item()) == S
    M = 3 * S
    mark = -7.0
    outs = [torch.full(s, mark, device=gpu) for s in ((M, 3), (M, 3), (M,), (M, 4), (M,))]

    def emit(cap):
        return lib.syn3r_gaussian_unpool_emit(L.ptr(pts), L.ptr(ls), L.ptr(o), L.ptr(c), L.ptr(i_gpu), n, S, cap, *[L.ptr(t) for t in outs],
                                              L.ptr(ws), ws.numel(), L.stream_ptr(gpu))
    assert emit(M - 1) == -1 and b"capacity" in lib.syn3r_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == mark).all()) for t in outs)
    assert emit(M) == 0
    for t, k in zip(outs, ("xyz", "scaling", "opacity", "rotation", "confidence")):
        assert np.array_equal(_np(t), exp[k]), k


# ------------------------------------------------------------------------------------------------ 8. trainer
def _gpu_trainer(n, seed, gpu, cams=(), **opt):
    """The model of tests/test_densify.py on the device, in front of an identity camera, Adam moment of Gaussian i = i + 1."""
    from syn3r_amd.gs.trainer import GaussianModel, GSTrainer, OptimizationParams
    g = np.random.default_rng(seed)
    xyz = g.normal(size=(n, 3)).astype(np.float32) * F32(0.5) + np.array([0, 0, 4], dtype=np.float32)
    log_s = np.log(g.uniform(0.002, 0.05, size=(n, 3))).astype(np.float32)
    rot = g.normal(size=(n, 4)).astype(np.float32)
    op = (g.normal(size=n) * 3).astype(np.float32)
    sh = (g.normal(size=(n, 16, 3)) * 0.3).astype(np.float32)
    gm = GaussianModel(xyz, log_s, rot, op, sh, device=gpu)
    gm.confidence = torch.from_numpy(g.uniform(0.1, 1.0, n).astype(np.float32)).to(gpu)
    tr = GSTrainer(gm, list(cams), OptimizationParams(**opt))
    for p in gm.parameters():
        m = torch.arange(1, n + 1, dtype=torch.float32, device=gpu).reshape(n, *([1] * (p.dim() - 1))).expand_as(p).clone()
        tr.optimizer.state[p] = {"step": 7, "exp_avg": m.clone(), "exp_avg_sq": 2 * m}
    gm.ensure_stats()
    gm.denom[:] = torch.from_numpy(g.integers(0, 5, (n, 1)).astype(np.float32)).to(gpu)
    gm.xyz_gradient_accum[:] = torch.from_numpy(g.uniform(0, 0.002, (n, 1)).astype(np.float32)).to(gpu) * gm.denom
    gm.max_radii2D[:] = torch.from_numpy(g.uniform(0, 30, n).astype(np.float32)).to(gpu)
    return tr


def _camera(gpu, H=48, W=64):
    from syn3r_amd.gs import Camera
    K = np.array([[W / (2 * math.tan(math.radians(30))), 0, W / 2], [0, W / (2 * math.tan(math.radians(30))), H / 2], [0, 0, 1]],
                 dtype=np.float32)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(2))
    return Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, image=target, data_device=gpu)


def test_trainer_proximity_unpool_appends_the_restated_rows(gpu):
    n, extent = 600, 2.0
    tr = _gpu_trainer(n, 5, gpu)
    gm = tr.gaussians
    before = {a: _np(getattr(gm, a)).copy() for a in tr.density._PARAM_ATTRS}
    conf0 = _np(gm.confidence).copy()
    dist, idx = graph_bruteforce(before["_xyz"])
    q = float(np.quantile(_score(dist), 0.8))
    tr.opt.proximity_dist_factor, tr.opt.proximity_scale_factor = q / extent, 0.01
    st, lt = float(tr.opt.proximity_dist_factor) * extent, math.log(0.01 * extent)
    exp, S, _, _ = unpool_restated(before["_xyz"], before["_scaling"], before["_opacity"], conf0, dist, idx, st, lt)
    assert 0.05 <= S / n <= 0.5
    m = tr.proximity_unpool(extent)
    assert m == 3 * S and gm._xyz.shape[0] == n + m
    for attr, key in (("_xyz", "xyz"), ("_scaling", "scaling"), ("_opacity", "opacity"), ("_rotation", "rotation")):
        got = _np(getattr(gm, attr))
        assert np.array_equal(got[:n], before[attr]), attr                # the old rows keep their values
        assert np.array_equal(got[n:], exp[key]), attr                    # the new rows, row for row
    assert np.array_equal(_np(gm.confidence), np.concatenate([conf0, exp["confidence"]]))
    feats = _np(gm._features)
    assert feats.shape == (n + m, 16, 3) and np.array_equal(feats[:n], before["_features"]) and not feats[n:].any()
    rot_new = _np(gm._rotation)[n:]
    assert (rot_new[:, 0] == 1).all() and not rot_new[:, 1:].any()
    for grp, p in zip(tr.optimizer.param_groups, gm.parameters()):
        assert grp["params"][0] is p
        stt = tr.optimizer.state[p]
        assert stt["step"] == 7 and stt["exp_avg"].shape == p.shape and stt["exp_avg_sq"].shape == p.shape
        first = _np(stt["exp_avg"]).reshape(n + m, -1)
        second = _np(stt["exp_avg_sq"]).reshape(n + m, -1)
        assert np.array_equal(first[:n, 0], np.arange(1, n + 1, dtype=np.float32)) and not first[n:].any()
        assert np.array_equal(second[:n, 0], 2 * np.arange(1, n + 1, dtype=np.float32)) and not second[n:].any()
    assert gm.xyz_gradient_accum.shape == (n + m, 1) and float(gm.xyz_gradient_accum.abs().sum()) == 0.0
    assert gm.denom.shape == (n + m, 1) and float(gm.denom.abs().sum()) == 0.0
    assert gm.max_radii2D.shape == (n + m,) and float(gm.max_radii2D.abs().sum()) == 0.0


def test_trainer_proximity_unpool_leaves_the_model_alone_without_sources(gpu):
    tr = _gpu_trainer(300, 6, gpu)
    gm = tr.gaussians
    tr.opt.proximity_dist_factor = 1e6
    params = list(gm.parameters())
    accum = gm.xyz_gradient_accum.clone()
    assert tr.proximity_unpool(2.0) == 0
    assert all(a is b for a, b in zip(params, gm.parameters())) and torch.equal(accum, gm.xyz_gradient_accum)
    assert _gpu_trainer(3, 7, gpu).proximity_unpool(2.0) == 0              # fewer than 4 Gaussians


def test_densify_and_prune_runs_the_unpooling_between_split_and_prune(gpu):
    n, extent, args = 600, 2.0, (0.0008, 0.05, 2.0, 20.0)
    cam = _camera(gpu)
    off = _gpu_trainer(n, 5, gpu, cams=[cam])
    # thresholds: the 0.8 quantile of the INPUT cloud's scores (restated) and a scale of 0.01
    q = float(np.quantile(_score(graph_bruteforce(_np(off.gaussians._xyz))[0]), 0.8))
    on = _gpu_trainer(n, 5, gpu, cams=[cam], use_proximity_densify=True, proximity_dist_factor=q / extent,
                      proximity_scale_factor=0.01 / extent)
    off.proximity_unpool = lambda e: pytest.fail("proximity_unpool reached with the flag off")
    c_off = off.densify_and_prune(*args)
    assert min(c_off) > 10 and off.last_unpooled == 0                     # clone, split and prune all fire
    seen = []
    orig = on.proximity_unpool

    def wrapped(e):
        seen.append((on.gaussians._xyz.shape[0], e))
        return orig(e)
    on.proximity_unpool = wrapped
    c_on = on.densify_and_prune(*args)
    print("flag off", c_off, "flag on", c_on, "unpooled", on.last_unpooled)
    assert c_on[:2] == c_off[:2] and c_on[2] >= c_off[2]
    assert seen == [(n + c_on[0] + c_on[1], extent)]                      # once, after the split, before the prune
    assert on.last_unpooled > 0 and on.last_unpooled % 3 == 0
    gm = on.gaussians
    n_now = gm._xyz.shape[0]
    assert n_now == n + c_on[0] + c_on[1] + on.last_unpooled - c_on[2]
    assert gm._features.shape[0] == n_now and gm.confidence.shape[0] == n_now and gm.max_radii2D.shape == (n_now,)
    for grp, p in zip(on.optimizer.param_groups, gm.parameters()):
        assert grp["params"][0] is p and on.optimizer.state[p]["exp_avg"].shape == p.shape
    loss = on.train_step(cam)
    assert torch.isfinite(loss) and torch.isfinite(on.render_view(cam)["render"]).all()


# ------------------------------------------------------------------------------------------------ 9. training run
def _thin_run(gpu, flag: bool):
    from oracle import raster_oracle as RO
    from syn3r_amd.gs import Camera, GaussianModel, GSTrainer, OptimizationParams

    def scene(N, seed):
        m, s, q, o, sh = RO.synthetic_gaussians(N, seed=seed, log_scale_mean=np.log(0.08))
        logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
        return GaussianModel(m, torch.log(s), q, logit, sh, device=gpu)

    H, W = 64, 96
    f = W / (2 * math.tan(math.radians(30)))
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=np.float32)
    cam0 = Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, data_device=gpu)
    target = GSTrainer(scene(1500, 11), [cam0]).render_view(cam0)["render"].detach()
    gm = scene(300, 12)                                                      # a thin initial model
    cam = Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, image=target, data_device=gpu)
    opt = OptimizationParams(iterations=120, position_lr=2e-3, densify_from_iter=10, densification_interval=20,
                             opacity_reset_interval=1000, densify_grad_threshold=3e-4, prune_min_opacity=0.02,
                             use_proximity_densify=flag, proximity_until_iter=60)
    tr = GSTrainer(gm, [cam], opt)
    extent = tr.cameras_extent()
    # factors from the INITIAL model: the 0.8 quantile of its scores and the median of its largest scales
    xyz, log_s = _np(gm._xyz), _np(gm._scaling)
    dist, idx = graph_bruteforce(xyz)
    opt.proximity_dist_factor = float(np.quantile(_score(dist), 0.8)) / extent
    opt.proximity_scale_factor = float(np.exp(np.median(log_s.max(axis=1)))) / extent
    st, lt = float(opt.proximity_dist_factor) * extent, math.log(float(opt.proximity_scale_factor) * extent)
    _, S, _, _ = unpool_restated(xyz, log_s, _np(gm._opacity), _np(gm.confidence), dist, idx, st, lt)
    assert 0.05 <= S / 300 <= 0.5, S
    return tr, cam, H, W


def test_training_with_unpooling_from_a_thin_model(gpu):
    from syn3r_amd import raster
    tr, cam, H, W = _thin_run(gpu, True)
    gm = tr.gaussians
    first = float(tr.train_step(cam))
    log = []
    orig = tr.densify_and_prune

    def recorded(*a):
        it = tr.iteration + 1
        r = orig(*a)
        log.append((it, r, tr.last_unpooled))
        return r
    tr.densify_and_prune = recorded
    last = tr.training(0, 0)
    print("densifications (iteration, (clone, split, prune), unpooled):", log, "loss", first, "->", last)
    assert [e[0] for e in log] == [20, 40, 60, 80, 100, 120]
    assert any(e[2] > 0 for e in log if e[0] < 60)
    assert all(e[2] == 0 for e in log if e[0] >= 60)
    n_now = gm._xyz.shape[0]
    assert n_now != 300 and gm._features.shape[0] == n_now and gm.confidence.shape[0] == n_now
    for grp, p in zip(tr.optimizer.param_groups, gm.parameters()):
        assert grp["params"][0] is p and tr.optimizer.state[p]["exp_avg"].shape == p.shape
    assert np.isfinite(last) and last < 0.8 * first, (first, last)
    assert tr.truncated_renders == 0
    assert not raster._pending and raster.capacity_key(gpu, n_now, H, W) in raster._capacity


def test_training_with_the_flag_off_never_calls_the_operator(gpu):
    tr, cam, _, _ = _thin_run(gpu, False)
    tr.proximity_unpool = lambda e: pytest.fail("proximity_unpool reached with the flag off")
    last = tr.training(0, 0)
    assert np.isfinite(last) and tr.last_unpooled == 0
