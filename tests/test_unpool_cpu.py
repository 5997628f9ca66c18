"""FSGS' proximity-guided Gaussian unpooling without a GPU: the launcher flag, the trainer's defaults, the host-side argument
checks of the C-ABI entries (syn3r_knn3_graph, syn3r_gaussian_unpool_count / _emit), which reject a call before any HIP work, and
that the density control does not reach the operator while the flag is off."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

E_INVALID, E_WORKSPACE = -1, -2
DIM_MAX = 1 << 24


@pytest.fixture(scope="module")
def lib():
    from syn3r_amd import _lib, build
    build.build()
    return _lib.load()


def test_launcher_declares_the_flag():
    from syn3r_amd import launch
    a = launch.parse(["--scenes", "x", "--use_proximity_densify", "1"])
    assert a.use_proximity_densify == 1
    assert "--use_proximity_densify" not in a.ignored_flags and a.ignored_flags == []
    assert launch.parse(["--scenes", "x"]).use_proximity_densify == 0
    assert "--use_proximity_densify" not in launch.FSGS_FLAGS
    # the form the reference's LLFF / DL3DV batch scripts pass, next to a flag that stays tolerated and ignored
    b = launch.parse(["--scenes", "x", "--use_proximity_densify", "0", "--sample_pseudo_interval", "1"])
    assert b.use_proximity_densify == 0 and b.ignored_flags == ["--sample_pseudo_interval", "1"]


def test_trainer_defaults_leave_the_feature_off():
    from syn3r_amd.gs import OptimizationParams
    o = OptimizationParams()
    assert o.use_proximity_densify is False
    assert (o.proximity_until_iter, o.proximity_dist_factor, o.proximity_scale_factor) == (2000, 5.0, 1.0)


def _err(lib):
    return lib.syn3r_last_error().decode()


def test_version_raised(lib):
    assert lib.syn3r_version() > 200


def test_graph_entry_rejects_bad_arguments(lib):
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 255) & ~255      # never dereferenced: every call below is rejected
    n = 64
    need = lib.syn3r_knn3_graph_workspace_bytes(n)
    assert need > 0 and need == lib.syn3r_knn3_workspace_bytes(n)
    for bad in (0, -1, DIM_MAX + 1):
        assert lib.syn3r_knn3_graph_workspace_bytes(bad) == 0

    def call(pts=p, n_=n, d=p, i=p, ws=p, wsb=need):
        return lib.syn3r_knn3_graph(pts, n_, d, i, ws, wsb, None)

    for kw in (dict(pts=None), dict(d=None), dict(i=None), dict(ws=None)):
        assert call(**kw) == E_INVALID and "null" in _err(lib), kw
    for bad in (3, 0, -7, DIM_MAX + 1):
        assert call(n_=bad) == E_INVALID and f"n={bad}" in _err(lib)
    assert call(wsb=need - 1) == E_WORKSPACE and "workspace" in _err(lib)
    assert call(ws=p + 16) == E_INVALID and "workspace" in _err(lib) and "aligned" in _err(lib)
    # the two older search entries answer a short workspace with E_INVALID (the header documents E_WORKSPACE for the graph and
    # unpooling entries only)
    assert lib.syn3r_knn3_mean_dist2(p, n, p, p, lib.syn3r_knn3_workspace_bytes(n) - 1, None) == E_INVALID and "workspace" in _err(lib)
    need64 = lib.syn3r_pcd_outlier_workspace_bytes(n)
    assert need64 > need
    assert lib.syn3r_pcd_statistical_outlier(p, n, 20, 3.0, p, p, p, p, need64 - 1, None) == E_INVALID and "workspace" in _err(lib)


def test_unpool_entries_reject_bad_arguments(lib):
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 255) & ~255
    n = 64
    need = lib.syn3r_gaussian_unpool_workspace_bytes(n)
    assert need > 0 and need % 256 == 0
    for bad in (0, -1, DIM_MAX + 1):
        assert lib.syn3r_gaussian_unpool_workspace_bytes(bad) == 0
    inf = float("inf")

    def count(d=p, ls=p, n_=n, st=1.0, lt=-inf, c=p, ws=p, wsb=need):
        return lib.syn3r_gaussian_unpool_count(d, ls, n_, st, lt, c, ws, wsb, None)

    for kw in (dict(d=None), dict(ls=None), dict(c=None), dict(ws=None)):
        assert count(**kw) == E_INVALID and "null" in _err(lib), kw
    for bad in (3, 0, -7, DIM_MAX + 1):
        assert count(n_=bad) == E_INVALID and f"n={bad}" in _err(lib)
    assert count(st=float("nan")) == E_INVALID and "NaN" in _err(lib)
    assert count(lt=float("nan")) == E_INVALID and "NaN" in _err(lib)
    assert count(wsb=need - 1) == E_WORKSPACE and "workspace" in _err(lib)
    assert count(ws=p + 16) == E_INVALID and "aligned" in _err(lib)

    names = ("xyz", "ls", "op", "conf", "idx", "o_xyz", "o_ls", "o_op", "o_rot", "o_conf", "ws")

    def emit(n_=n, s=5, cap=15, wsb=need, **kw):
        a = {k: kw.get(k, p) for k in names}
        return lib.syn3r_gaussian_unpool_emit(a["xyz"], a["ls"], a["op"], a["conf"], a["idx"], n_, s, cap, a["o_xyz"], a["o_ls"],
                                              a["o_op"], a["o_rot"], a["o_conf"], a["ws"], wsb, None)

    for k in names:
        assert emit(**{k: None}) == E_INVALID and "null" in _err(lib), k
    for bad in (3, 0, -7, DIM_MAX + 1):
        assert emit(n_=bad) == E_INVALID and f"n={bad}" in _err(lib)
    assert emit(s=5, cap=14) == E_INVALID and "capacity" in _err(lib)          # one row short
    assert emit(s=-1) == E_INVALID and "n_sources" in _err(lib)
    assert emit(s=n + 1, cap=3 * n + 3) == E_INVALID and "n_sources" in _err(lib)
    assert emit(wsb=need - 1) == E_WORKSPACE and "workspace" in _err(lib)
    assert emit(ws=p + 16) == E_INVALID and "aligned" in _err(lib)


def test_wrappers_reject_cpu_tensors():
    from syn3r_amd import _lib
    from syn3r_amd.gs.train_ops import knn3_graph, proximity_unpool
    x = torch.rand(16, 3)
    with pytest.raises(_lib.Syn3rError):
        knn3_graph(x)
    with pytest.raises(_lib.Syn3rError):
        proximity_unpool(x, torch.zeros(16, 3), torch.zeros(16), torch.ones(16), 0.1, -float("inf"))


def _cpu_trainer(n, seed, **opt):
    from syn3r_amd.gs.trainer import GaussianModel, GSTrainer, OptimizationParams
    g = np.random.default_rng(seed)
    gm = GaussianModel(g.normal(size=(n, 3)).astype(np.float32), np.log(g.uniform(0.002, 0.05, size=(n, 3))).astype(np.float32),
                       g.normal(size=(n, 4)).astype(np.float32), (g.normal(size=n) * 3).astype(np.float32),
                       g.normal(size=(n, 16, 3)).astype(np.float32), device="cpu")
    tr = GSTrainer(gm, [], OptimizationParams(**opt))
    gm.ensure_stats()
    gm.denom[:] = torch.from_numpy(g.integers(1, 5, (n, 1)).astype(np.float32))
    gm.xyz_gradient_accum[:] = torch.from_numpy(g.uniform(0, 0.002, (n, 1)).astype(np.float32)) * gm.denom
    return tr


def test_flag_off_never_reaches_the_operator():
    """Default options: densify_and_prune runs on CPU tensors as before, the unpooling is not called, last_unpooled stays 0."""
    tr = _cpu_trainer(300, 3)

    def boom(extent):
        raise AssertionError("proximity_unpool reached with the flag off")
    tr.proximity_unpool = boom
    assert tr.last_unpooled == 0
    n_clone, n_split, n_prune = tr.densify_and_prune(0.0008, 0.05, 2.0, 20.0)
    assert n_clone + n_split > 0
    assert tr.last_unpooled == 0 and tr.gaussians._xyz.shape[0] == 300 + n_clone + n_split - n_prune


def test_flag_on_calls_the_operator_only_before_its_last_iteration():
    """The schedule gate, with the operator replaced by a stub (no GPU): called while iteration + 1 < proximity_until_iter."""
    tr = _cpu_trainer(300, 4, use_proximity_densify=True, proximity_until_iter=50)
    seen = []
    tr.proximity_unpool = lambda extent: seen.append((tr.iteration, extent)) or 0
    tr.iteration = 48
    tr.densify_and_prune(0.0008, 0.05, 2.0, None)
    assert seen == [(48, 2.0)] and tr.last_unpooled == 0
    tr.gaussians.ensure_stats()
    tr.iteration = 49
    tr.densify_and_prune(0.0008, 0.05, 2.0, None)
    assert seen == [(48, 2.0)]


def test_trainer_op_refuses_a_cpu_model():
    """GSTrainer.proximity_unpool has no CPU fallback; fewer than 4 Gaussians is a quiet 0."""
    from syn3r_amd import _lib
    tr = _cpu_trainer(20, 5)
    with pytest.raises(_lib.Syn3rError):
        tr.proximity_unpool(1.0)
    assert _cpu_trainer(3, 6).proximity_unpool(1.0) == 0
