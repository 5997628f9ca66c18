"""The multi-view photometric reprojection term without a GPU: the float64 restatement (tests/reproj_ref.py) against itself, the host
side (syn3r_amd/gs/reproj.py: relative views, the source rule, the cache), the options and flags, the argument checks of the C-ABI
entries (rejected before any HIP call), and the abstract descent design that gives the GPU copy of that test its meaning."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import reproj_ref as R

ROOT = Path(__file__).resolve().parents[1]
E_INVALID, E_WORKSPACE = -1, -2
ENTRIES = ("syn3r_photo_reproj_workspace_bytes", "syn3r_photo_reproj_loss", "syn3r_photo_reproj_loss_backward",
           "syn3r_photo_reproj_loss_step")
F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    from syn3r_amd import _lib, build
    build.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ the restatement against itself
@pytest.mark.parametrize("key", [(37, 53, 1, 1), (37, 53, 2, 2), (37, 53, 4, 3)], ids=str)
def test_analytic_gradient_is_autograd_through_depth_over_alpha(key):
    """The closed forms (cancellation-free dq/dz, the bilinear cell's derivative, sgn, g_depth = dL/dz / a, g_alpha = -dL/dz z / a)
    against float64 autograd of the torch restatement, which differentiates D / a itself: 1e-12 of the largest gradient."""
    c = R.make_case(*key)
    r = R.term(c["depth"], c["alpha"], c["target"], c["sources"], c["views"], 0.7, 0.5, autograd=True)
    assert r.n_live > 0.5 * key[0] * key[1]
    for name, got, want in (("depth", r.g_depth, r.ag_depth), ("alpha", r.g_alpha, r.ag_alpha)):
        tol = 1e-12 * float(want.abs().max())
        assert float(want.abs().max()) > 0 and float((got - want).abs().max()) <= tol, name
        assert not got[~r.live].any() and not want[~r.live].any()


def test_analytic_gradient_is_the_central_difference_away_from_the_kinks():
    """Every pixel's e depends on its own depth alone (N_live is held constant), so ONE pair of evaluations at D +- h gives every
    pixel's central difference.  Compared where the chosen source, its bilinear cell and the signs of its channel differences are the
    same at D - h, D and D + h (away from the kinks); the term is piecewise smooth with bounded second derivative there: 1e-6 of the
    largest gradient for h = 1e-6 relative.  (fp32 inputs cannot carry h: the perturbed depth is handed over in float64.)"""
    key = (37, 53, 2, 2)
    c = R.make_case(*key)
    D = c["depth"].to(F64)
    h = 1e-6 * D.clamp(min=1e-3)
    args = (c["alpha"], c["target"], c["sources"], c["views"], 1.0, 0.5)
    r0, rm, rp = R.term(D, *args), R.term(D - h, *args), R.term(D + h, *args)

    def signature(r):
        arg = r.src.clamp(min=0)
        pick = lambda lst: torch.stack(list(lst)).gather(0, arg[None])[0]
        qx, qy = pick([q[0] for q in r.q]), pick([q[1] for q in r.q])
        sg = torch.stack([torch.sign(d) for d in r.diff]).gather(0, arg[None, None].expand(1, 3, *arg.shape))[0]
        return r.src, qx.floor(), qy.floor(), sg
    same = r0.live.clone()
    for a, b in zip(signature(r0), signature(rm)):
        same &= (a == b) if a.dim() == 2 else (a == b).all(0)
    for a, b in zip(signature(r0), signature(rp)):
        same &= (a == b) if a.dim() == 2 else (a == b).all(0)
    assert float(same.sum()) > 0.9 * r0.n_live
    fd = (rp.e - rm.e) / (2 * h) / r0.n_live
    err = (fd - r0.g_depth).abs()[same]
    assert float(err.max()) <= 1e-6 * float(r0.g_depth.abs().max())


def _identity_views(H, W, t=(0.0, 0.0, 0.0)):
    k = R.case_intrinsics(H, W)
    return k.astype(np.float32), np.concatenate([np.eye(3).reshape(9), t, k]).astype(np.float32)[None]


def test_identity_pose_compares_the_pixel_with_itself():
    H, W = 9, 14
    g = torch.Generator().manual_seed(2)
    It, Is = R.smooth_image(H, W, g), R.smooth_image(H, W, g)
    D, a = 1.0 + torch.rand(H, W, generator=g), torch.ones(H, W)
    r = R.term(D, a, It, [Is], _identity_views(H, W), 1.0, 0.5, autograd=True)
    want = (Is.to(F64) - It.to(F64)).abs().mean(0)
    assert r.n_live == H * W and float((r.e - want).abs().max()) <= 1e-13
    assert not r.g_depth.any() and not r.g_alpha.any()            # t = 0: the cancellation-free dq/dz is an exact 0
    assert float(r.ag_depth.abs().max()) <= 1e-15 and float(r.ag_alpha.abs().max()) <= 1e-15      # (autograd: the quotient rule, to rounding)


def test_x_translation_is_the_stereo_disparity():
    H, W, b = 7, 40, 0.11
    g = torch.Generator().manual_seed(4)
    z = 2.0 + torch.rand(H, W, generator=g)
    tk, table = _identity_views(H, W, (b, 0.0, 0.0))
    r = R.term(z, torch.ones(H, W), torch.rand(3, H, W, generator=g), [torch.rand(3, H, W, generator=g)], (tk, table), 1.0, 0.5)
    xs = torch.arange(W, dtype=F64)[None].expand(H, W)
    fx = float(np.float32(tk[0]))
    want = xs + fx * float(np.float32(b)) / z.to(F64)
    assert float((r.q[0][0] - want).abs().max()) <= 1e-12 * W
    ys = torch.arange(H, dtype=F64)[:, None].expand(H, W)
    assert float((r.q[0][1] - ys).abs().max()) <= 1e-12 * H


def test_cancellation_free_dq_dz_is_the_quotient_rule():
    """dq_x/dz = fx (A_x X_z - X_x A_z) / X_z^2 with X = z A + t: the z A_x A_z terms cancel, fx (A_x t_z - A_z t_x) / X_z^2 is left."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        A, t, z, f = rng.normal(size=3), rng.normal(size=3), rng.uniform(0.5, 5.0), rng.uniform(10, 900)
        X = z * A + t
        if abs(X[2]) < 0.05:
            continue
        quotient = f * (A[0] * X[2] - X[0] * A[2]) / X[2] ** 2
        free = f * (A[0] * t[2] - A[2] * t[0]) / X[2] ** 2
        h = 1e-6
        fd = (f * (z + h) * A[0] + f * t[0]) / ((z + h) * A[2] + t[2]) - (f * (z - h) * A[0] + f * t[0]) / ((z - h) * A[2] + t[2])
        scale = abs(f) * (abs(A[0] * X[2]) + abs(X[0] * A[2])) / X[2] ** 2
        assert abs(quotient - free) <= 1e-12 * scale
        assert abs(fd / (2 * h) - free) <= 1e-5 * max(scale, 1.0) / min(1.0, abs(X[2])) ** 2


def test_empty_and_dead_cases():
    H, W = 5, 6
    g = torch.Generator().manual_seed(6)
    It, Is = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
    v = _identity_views(H, W)
    r = R.term(torch.ones(H, W), torch.zeros(H, W), It, [Is], v, 1.0, 0.5, autograd=True)
    assert r.n_live == 0 and r.loss == 0.0 and r.parts == [0.0, 0.0, 0.0, 0.0] and not r.g_depth.any() and not r.ag_alpha.any()
    # a source that sees nothing (behind the camera): dead although alpha and depth are fine
    tk, table = _identity_views(H, W, (0.0, 0.0, -50.0))
    r = R.term(torch.ones(H, W), torch.ones(H, W), It, [Is], (tk, table), 1.0, 0.5)
    assert r.n_live == 0 and bool((r.src == -1).all())
    # the lowest source wins a tie
    r = R.term(torch.ones(H, W), torch.ones(H, W), It, [Is, Is.clone()], (v[0], np.concatenate([v[1], v[1]])), 1.0, 0.5)
    assert bool((r.src == 0).all())


def test_reference_cases_stay_inside_the_left_out_share():
    """The condition the GPU comparison rests on, checked with the float64 restatement ALONE: the pixels within an fp32 margin of a kink
    are at most 2 % of every case (none at all where 2 % is less than a pixel), and every case has live pixels, dead pixels of both
    kinds and, for S > 1, every source in use."""
    for key in R.CASES:
        H, W, S, _ = key
        c, r, (amb, unsure) = R.reference(key)
        out = int((amb | unsure).sum())
        assert out <= R.MAX_LEFT_OUT * H * W, (key, out)
        assert 0 < r.n_live < H * W
        if H * W > 100:
            assert bool((r.live0 & ~r.live).any()) and bool((~r.live0).any())            # no valid source / low alpha
            assert all(int((r.src == s).sum()) > 0 for s in range(S))
    assert R.trips(*R.SECOND_TRIP) == 2 and R.trips(R.SECOND_TRIP[0] - 1, R.SECOND_TRIP[1]) == 1


def test_descent_design_recovers_the_plane_in_float64():
    """The abstract design (tests/reproj_ref.py plane_design): from z = 1.08 z* plain gradient descent on the per-pixel z shrinks
    mean |z - z*| below half its start.  A condition on the DESIGN: the GPU test runs the same loop on the operator and is held to
    this float64 loop's result."""
    d = R.plane_design()
    assert d["lam_px"] >= 4.0 * d["err_px"] and d["lam_px"] >= 6.0            # resolvable by the pixel lattice, start inside the basin
    _, e0, e1 = R.descend(d, R.ref_step(d), R.descent_rate(d))
    print(f"descent design: mean |z - z*| {e0:.5f} -> {e1:.5f} ({e1 / e0:.3f} of the start)")
    assert e1 < 0.5 * e0


# ------------------------------------------------------------------------------------------------------------------- host side
def _cams(n=4, H=33, W=50, seed=0, dx=0.1):
    from syn3r_amd.gs import Camera
    g = torch.Generator().manual_seed(seed)
    K = np.array([[40.0, 0, W / 2], [0, 44.0, H / 2], [0, 0, 1]], dtype=np.float32)
    cams = []
    for k in range(n):
        w2c = np.eye(4, dtype=np.float32)
        w2c[0, 3] = dx * k
        cams.append(Camera.from_w2c(w2c, K, H, W, image=torch.rand(3, H, W, generator=g), data_device="cpu"))
    return cams, K


def _rot_y(deg):
    th = math.radians(deg)
    return np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]])


def test_relative_view_is_the_float64_matrix_product():
    from syn3r_amd.gs import reproj as P
    cams, _ = _cams(2)
    rng = np.random.default_rng(1)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    cams[0].set_pose(_rot_y(7.0), np.array([0.3, -0.1, 0.2]))
    cams[1].set_pose(q, np.array([-0.2, 0.05, 0.4]))
    t, s = cams
    v = P.relative_view(t, s)
    w2c = lambda c: c.world_view_transform.double().numpy().T            # the matrix the rasteriser projects with
    rel = w2c(s) @ np.linalg.inv(w2c(t))
    assert np.abs(v[:9].reshape(3, 3) - rel[:3, :3]).max() <= 1e-6 and np.abs(v[9:12] - rel[:3, 3]).max() <= 1e-6
    # and to float64 rounding, from the cameras' own R, T (fp32 values, so R is orthonormal to 1e-7 only: the INVERSE, not R^T)
    def own(c):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = c.R.astype(np.float64).T, c.T.astype(np.float64)
        return m
    rel = np.linalg.solve(own(t).T, own(s).T).T                       # own(s) own(t)^-1
    assert np.abs(v[:9].reshape(3, 3) - rel[:3, :3]).max() <= 1e-14 and np.abs(v[9:12] - rel[:3, 3]).max() <= 1e-14
    Rt, Rs, Tt, Ts = t.R.astype(np.float64), s.R.astype(np.float64), t.T.astype(np.float64), s.T.astype(np.float64)
    M = Rs.T @ Rt
    assert np.abs(v[:9].reshape(3, 3) - M).max() <= 1e-6 and np.abs(v[9:12] - (Ts - M @ Tt)).max() <= 1e-6
    W, H = s.image_width, s.image_height
    k = [W / (2 * math.tan(s.FoVx / 2)), H / (2 * math.tan(s.FoVy / 2)), (W - 1) / 2, (H - 1) / 2]
    assert np.abs(v[12:] - k).max() <= 1e-12 and abs(k[0] - 40.0) <= 1e-4 and abs(k[1] - 44.0) <= 1e-4
    assert v.dtype == np.float64 and P.intrinsics(t).dtype == np.float64
    # a point of the world lands where the two cameras say
    Xw = np.array([0.4, -0.3, 3.0, 1.0])
    Xt, Xs = w2c(t) @ Xw, w2c(s) @ Xw
    assert np.abs(v[:9].reshape(3, 3) @ Xt[:3] + v[9:12] - Xs[:3]).max() <= 1e-5


def test_source_rule():
    from syn3r_amd.gs import Camera
    from syn3r_amd.gs import reproj as P
    cams, K = _cams(5)                                   # centres at x = 0, -0.1, -0.2, -0.3, -0.4 (w2c translation +0.1 k)
    t = cams[2]
    pick = lambda **kw: [cams.index(c) for c in P.select_sources(t, cams, kw.get("n", 2), kw.get("angle", 45.0))]
    assert pick() == [1, 3]                              # the two nearest, a distance tie: list order; never the target itself
    assert pick(n=4) == [1, 3, 0, 4] and pick(n=1) == [1] and pick(n=0) == []
    # the angle gate: camera 1 turned by 50 degrees drops out at 45, stays at 60
    cams[1].set_pose(_rot_y(50.0), cams[1].T)
    assert 1 not in pick(n=4) and 1 in pick(n=4, angle=60.0)
    cams[1].set_pose(np.eye(3), cams[1].T)
    # the distance order follows a moved camera (its centre, not its place in the list)
    cams[0].set_pose(np.eye(3), np.array([0.21, 0.0, 0.0]))            # centre x = -0.21: 0.01 from the target
    assert pick() == [0, 1]
    # a camera of another size, or without an image, is no candidate
    H, W = t.image_height, t.image_width
    odd = Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W + 1, image=torch.rand(3, H, W + 1), data_device="cpu")
    blank = Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, data_device="cpu")
    assert P.select_sources(t, [odd, blank, t], 2, 45.0) == []
    assert P.select_sources(t, [t], 2, 45.0) == []


def test_cache_follows_poses_and_the_camera_list():
    from syn3r_amd.gs import reproj as P
    cams, _ = _cams(4)
    cache = P.ReprojCache()
    a = cache.get(cams[1], cams, 2, 45.0)
    assert cache.builds == 1 and cache.get(cams[1], cams, 2, 45.0) is a and cache.builds == 1
    images, views, srcs = a
    assert srcs == [cams[0], cams[2]] and images[0] is cams[0].original_image
    assert views.table.dtype == np.float32 and views.table.shape == (2, 16) and views.target_k.shape == (4,)
    assert np.array_equal(views.table[1], P.relative_view(cams[1], cams[2]).astype(np.float32))
    # a moved SOURCE (set_pose makes new tensors), a moved target, another list, other options: each rebuilds
    cams[2].set_pose(cams[2].R, cams[2].T + np.float32(0.01))
    b = cache.get(cams[1], cams, 2, 45.0)
    assert cache.builds == 2 and b is not a and not np.array_equal(b[1].table, views.table)
    cams[1].set_pose(cams[1].R, cams[1].T + np.float32(0.01))
    cache.get(cams[1], cams, 2, 45.0)
    assert cache.builds == 3
    cache.get(cams[1], cams[:3], 2, 45.0)
    assert cache.builds == 4
    cache.get(cams[1], cams[:3], 1, 45.0)
    assert cache.builds == 5 and cache.get(cams[1], cams[:3], 1, 45.0) is not None and cache.builds == 5
    # a target without a source: None, cached as such
    assert cache.get(cams[0], cams[:1], 2, 45.0) is None and cache.get(cams[0], cams[:1], 2, 45.0) is None and cache.builds == 6
    # entries of cameras that left the scene are dropped (they hold the cameras and their images alive)
    import weakref
    gone = weakref.ref(cams[1].original_image)
    cache.retain([cams[0], cams[2], cams[3]])
    assert set(cache._entries) == {id(cams[0])}
    cache.retain([])
    old = cams.pop(1)
    del old, a, b, images, views, srcs
    assert gone() is None and not cache._entries


def _cpu_trainer(n_cams=3, **opt_kw):
    from syn3r_amd.gs import GSTrainer, OptimizationParams
    from syn3r_amd.gs.gaussian_model import GaussianModel
    g = torch.Generator().manual_seed(0)
    r = lambda *shape: torch.randn(*shape, generator=g)
    gm = GaussianModel(r(6, 3), r(6, 3), r(6, 4), r(6), r(6, 4, 3), sh_degree=1, device="cpu")
    cams, _ = _cams(n_cams)
    return GSTrainer(gm, cams, OptimizationParams(iterations=5, **opt_kw)), cams


def test_trainer_chooses_targets_and_keeps_the_term_out_of_checkpoints(tmp_path):
    tr, cams = _cpu_trainer()
    assert tr._reproj_sources(cams[0]) is None and tr.reproj.builds == 0            # off: nothing is asked of the cache
    tr.opt.reproj_weight = 0.1
    got = tr._reproj_sources(cams[1])
    assert got is not None and got[2] == [cams[0], cams[2]] and tr.reproj.builds == 1
    cams[2].is_pseudo = True                                # sources are input views only; "train" targets exclude pseudo-views
    assert tr._reproj_sources(cams[1])[2] == [cams[0]] and tr._reproj_sources(cams[2]) is None
    tr.opt.reproj_cameras = "pseudo"
    assert tr._reproj_sources(cams[1]) is None and tr._reproj_sources(cams[2])[2] == [cams[1], cams[0]]
    tr.opt.reproj_cameras = "all"
    assert tr._reproj_sources(cams[1]) is not None and tr._reproj_sources(cams[2]) is not None
    tr.opt.reproj_from_iter = 3
    assert tr._reproj_sources(cams[1]) is None
    tr.iteration = 3
    assert tr._reproj_sources(cams[1]) is not None
    tr.opt.reproj_max_angle = 45.0
    cams[0].set_pose(_rot_y(80.0), cams[0].T)               # the only input view besides the target turns away: no source, term skipped
    assert tr._reproj_sources(cams[1]) is None
    tr.opt.reproj_cameras = "none"
    with pytest.raises(ValueError, match="reproj_cameras"):
        tr._reproj_sources(cams[1])
    tr.opt.reproj_cameras = "all"
    tr.scene.model_path = str(tmp_path)
    state, _ = torch.load(tr.save_checkpoint(1), weights_only=True)
    assert not any("reproj" in k for k in state)


def test_options_flags_and_bad_values():
    from syn3r_amd import launch
    from syn3r_amd.gs import OptimizationParams
    o = OptimizationParams()
    assert (o.reproj_weight, o.reproj_sources, o.reproj_cameras, o.reproj_alpha_min, o.reproj_max_angle, o.reproj_from_iter) == \
        (0.0, 2, "train", 0.5, 45.0, 0)
    a = launch.parse(["--scenes", "x", "--reproj_weight", "0.25", "--reproj_sources", "3", "--reproj_cameras", "all", "--reproj_alpha_min",
                      "0.6", "--reproj_max_angle", "30", "--reproj_from_iter", "200"])
    assert not a.ignored_flags
    n = launch.apply_trainer_flags(OptimizationParams(), a)
    assert (n.reproj_weight, n.reproj_sources, n.reproj_cameras, n.reproj_alpha_min, n.reproj_max_angle, n.reproj_from_iter) == \
        (0.25, 3, "all", 0.6, 30.0, 200)
    assert launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x"])) == OptimizationParams()
    for bad in (["--reproj_cameras", "test"], ["--reproj_sources", "5"], ["--reproj_sources", "0"], ["--reproj", "0.5"],
                ["--reproj_weight", "much"]):
        with pytest.raises(SystemExit):
            launch.parse(["--scenes", "x"] + bad)
    for bad in (["--reproj_weight", "-1"], ["--reproj_weight", "nan"], ["--reproj_alpha_min", "0"], ["--reproj_alpha_min", "1.5"],
                ["--reproj_max_angle", "0"], ["--reproj_max_angle", "200"], ["--reproj_from_iter", "-1"]):
        with pytest.raises(ValueError, match=bad[0][2:]):
            launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x"] + bad))
    for kw in (dict(reproj_cameras="test"), dict(reproj_sources=5), dict(reproj_alpha_min=0.0), dict(reproj_weight=-0.1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            _cpu_trainer(**kw)


def test_exports_header_and_signatures():
    from syn3r_amd import _lib, build
    from syn3r_amd.gs import train_ops
    for name in ("photo_reprojection_loss", "photo_reprojection_loss_step", "photo_reprojection_records"):
        assert callable(getattr(train_ops, name))
    header = (ROOT / "include" / "syn3r_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\(", header) and name in _lib.SIGNATURES, name
    assert "reproj.hip" in build.STRICT_FP and (ROOT / "syn3r_amd" / "csrc" / "reproj.hip").exists()
    assert "UNPINNED" in header[header.index("Multi-view photometric reprojection"):header.index(ENTRIES[0] + "(")]
    src = (ROOT / "syn3r_amd" / "csrc" / "reproj.hip").read_text()
    assert "atomic" not in src.split("#include")[1]                 # no float atomics (the word appears in the header comment alone)
    assert '#include "plane_pass.h"' in src                            # the walk, the block rows and their sum live there: nor there
    assert "atomic" not in (ROOT / "syn3r_amd" / "csrc" / "plane_pass.h").read_text()
    assert f"kRpMaxBlocks = {R.MAX_BLOCKS};" in src and f"kRpThreads = {R.THREADS};" in src
    with pytest.raises(_lib.Syn3rError):                               # no CPU fallback
        train_ops.photo_reprojection_loss(torch.rand(4, 4), torch.rand(4, 4), torch.rand(3, 4, 4), [torch.rand(3, 4, 4)],
                                          _identity_views(4, 4))


def test_entries_reject_bad_arguments(lib):
    err = lambda: lib.syn3r_last_error().decode()
    buf = (ctypes.c_char * (1 << 20))()
    base = (ctypes.cast(buf, ctypes.c_void_p).value + 255) & ~255
    H, W, S = 8, 12, 2
    plane = H * W * 4
    d, a, tgt, s0, s1, gd, ga, parts = (base + 4096 * k for k in range(8))          # never dereferenced: every call below is rejected
    ws = base + 4096 * 16
    wsb = lib.syn3r_photo_reproj_workspace_bytes
    need = wsb(H, W, S)
    assert need >= 16384 + 8 * H * W and need % 256 == 0 and need <= 4096 * 8
    side = 1 << 15
    for bad in ((1, W, S), (H, 1, S), (0, W, S), (H, -1, S), (side + 1, W, S), (H, W, 0), (H, W, 5), (H, W, -1), (2 ** 31 - 1,) * 3):
        assert wsb(*bad) == 0, bad
    assert wsb(2, 2, 1) > 0 and wsb(side, side, 4) == 16384 + 8 * side * side
    srcs = (ctypes.c_void_p * 4)(s0, s1, s0, s1)
    views = (ctypes.c_float * 64)(*([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, 0, 0, 10, 10, 5.5, 3.5] * 4))
    tk = (ctypes.c_float * 4)(10, 10, 5.5, 3.5)

    def value(d_=d, a_=a, t_=tgt, srcs_=srcs, views_=views, tk_=tk, geom=(H, W, S), weight=1.0, amin=0.5, parts_=parts, ws_=ws, wsb_=need,
              gd_=gd, accd=0, ga_=ga, acca=0):
        return lib.syn3r_photo_reproj_loss(d_, a_, t_, srcs_, views_, tk_, *geom, weight, amin, parts_, ws_, wsb_, None)

    def step(d_=d, a_=a, t_=tgt, srcs_=srcs, views_=views, tk_=tk, geom=(H, W, S), weight=1.0, amin=0.5, parts_=parts, ws_=ws, wsb_=need,
             gd_=gd, accd=0, ga_=ga, acca=0):
        return lib.syn3r_photo_reproj_loss_step(d_, a_, t_, srcs_, views_, tk_, *geom, weight, amin, None, parts_, gd_, accd, ga_, acca, ws_,
                                                wsb_, None)

    def bwd(d_=d, a_=a, t_=tgt, srcs_=srcs, views_=views, tk_=tk, geom=(H, W, S), weight=1.0, amin=0.5, parts_=parts, ws_=ws, wsb_=need,
            gd_=gd, accd=0, ga_=ga, acca=0):
        return lib.syn3r_photo_reproj_loss_backward(d_, a_, *geom, weight, amin, None, ws_, wsb_, gd_, accd, ga_, acca, None)

    for call in (value, step, bwd):
        for kw in (dict(d_=None), dict(a_=None), dict(ws_=None)):
            assert call(**kw) == E_INVALID and "null" in err(), kw
        for geom in ((1, W, S), (H, 1, S), (0, W, S), (H, -3, S), (side + 1, W, S), (H, W, 0), (H, W, 5), (H, W, -2), (2 ** 31 - 1,) * 3):
            assert call(geom=geom) == E_INVALID and "H=" in err() and "S=" in err(), geom
        for w in (float("nan"), float("inf")):
            assert call(weight=w) == E_INVALID and "weight" in err()
        for m in (float("nan"), 0.0, -0.5, float("inf")):
            assert call(amin=m) == E_INVALID and "alpha_min" in err()
        assert call(ws_=ws + 4) == E_INVALID and "aligned" in err()
        assert call(wsb_=need - 1) == E_WORKSPACE and "workspace" in err()
    for call in (value, step):
        for kw in (dict(t_=None), dict(srcs_=None), dict(views_=None), dict(tk_=None), dict(parts_=None)):
            assert call(**kw) == E_INVALID and "null" in err(), kw
        assert call(srcs_=(ctypes.c_void_p * 4)(s0, None, s0, s0)) == E_INVALID and "source 1" in err()
        bad_views = (ctypes.c_float * 64)(*views)
        bad_views[20] = float("nan")
        assert call(views_=bad_views) == E_INVALID and "view 1" in err()
        assert call(tk_=(ctypes.c_float * 4)(0, 10, 5.5, 3.5)) == E_INVALID and "focal" in err()
        assert call(tk_=(ctypes.c_float * 4)(10, 10, float("inf"), 3.5)) == E_INVALID and "intrinsics" in err()
        assert call(parts_=parts + 4) == E_INVALID and "parts" in err()
        assert call(ws_=d - 256, wsb_=need + 4096) == E_INVALID and "aliases" in err()          # the workspace over the depth
    for call in (step, bwd):
        for kw in (dict(accd=2), dict(acca=-1), dict(accd=256)):
            assert call(**kw) == E_INVALID and "accumulate" in err(), kw
        assert call(gd_=None) == E_INVALID and "null" in err() and call(ga_=None) == E_INVALID and "null" in err()
        for g in (d, d + 4, d + plane - 4, a, a - plane + 4, ws, ws + need - 4):
            assert call(gd_=g) == E_INVALID and "aliases" in err(), g - base
            assert call(ga_=g) == E_INVALID and "aliases" in err(), g - base
        assert call(ga_=gd) == E_INVALID and "overlap" in err() and call(ga_=gd + plane - 4) == E_INVALID and "overlap" in err()
    for g in (tgt, tgt + 3 * plane - 4, tgt - plane + 4, s0, s1 + 3 * plane - 4):          # the step entry sees the images as well
        assert step(gd_=g) == E_INVALID and "aliases" in err(), g - base
        assert step(ga_=g) == E_INVALID and "aliases" in err(), g - base
