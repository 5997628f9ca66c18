"""Camera-pose refinement in the trainer (`OptimizationParams.pose_opt`): recovery of perturbed poses on a synthetic scene, "off is the
old path", and the bookkeeping (camera-list changes, checkpoints, the 3D filter's camera table)."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

from oracle import raster_oracle as RO  # noqa: E402

pytestmark = pytest.mark.gpu

H = W = 64
XIS = ((0.10, -0.05, 0.20, 0.08, -0.12, 0.05), (-0.15, 0.08, 0.10, -0.06, 0.10, -0.04), (0.05, 0.12, -0.10, 0.10, 0.05, 0.09))
DELTA = (0.02, -0.015, 0.01, 0.012, -0.01, 0.015)        # 1.24 degrees and 0.0269 units
FROZEN = dict(position_lr=0.0, feature_lr=0.0, opacity_lr=0.0, scaling_lr=0.0, rotation_lr=0.0)


def make_model(N, dev, seed=5):
    from syn3r_amd.gs import GaussianModel
    m, s, q, o, sh = RO.synthetic_gaussians(N, seed=seed, log_scale_mean=np.log(0.04))
    o = o.clamp(1e-3, 1 - 1e-3)
    return GaussianModel(m, torch.log(s), q, torch.log(o / (1 - o)), sh[:, :4].contiguous(), sh_degree=1, device=dev)


def intrinsics():
    fx = W / (2 * math.tan(math.radians(30)))
    return np.array([[fx, 0, W / 2], [0, fx, H / 2], [0, 0, 1]], dtype=np.float32)


def pose_error(cam, true_w2c):
    """(degrees, units) of E = M M_true^-1"""
    from syn3r_amd.gs.pose import camera_w2c
    E = camera_w2c(cam) @ np.linalg.inv(true_w2c)
    R = E[:3, :3]
    skew = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])        # sin(angle) axis: exact for small angles
    ang = math.degrees(math.atan2(float(np.linalg.norm(skew)), (np.trace(R) - 1.0) / 2.0))
    return ang, float(np.linalg.norm(E[:3, 3]))


def make_trainer(dev, opt_kw, n=600, perturbed=(1, 2), tmp=None):
    """three cameras at Exp(XIS[k]) with the images the trainer's own rasteriser renders THERE; cameras `perturbed` then start at
    Exp(DELTA) true.  -> (trainer, cameras, true w2c matrices)"""
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    from syn3r_amd.gs.pose import se3_exp
    gm, K = make_model(n, dev), intrinsics()
    truth = [se3_exp(x) for x in XIS]
    cams = [Camera.from_w2c(M.astype(np.float32), K, H, W, image=torch.zeros(3, H, W), data_device=dev) for M in truth]
    tr = GSTrainer(gm, cams, OptimizationParams(iterations=10, spatial_lr_scale=1.0, **FROZEN, **opt_kw), model_path=tmp)
    with torch.no_grad():
        for c in cams:
            c.original_image = tr.render_view(c)["render"].clamp(0, 1).detach().clone()
    for k in perturbed:
        M = se3_exp(DELTA) @ truth[k]
        cams[k].set_pose(M[:3, :3].T, M[:3, 3])
    return tr, cams, truth


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("interval", [1, 3])
def test_pose_recovery(interval, gpu, measurements):
    """600 frozen Gaussians, three 64 x 64 cameras, cameras 1 and 2 start 1.24 degrees / 0.027 units off; 150 updates per moved
    camera at both rates 1e-3.  The float64 oracle with an L1 loss reaches 0.003 - 0.005 degrees / 7 - 8e-5 from there; required on the
    device: both errors of both cameras at most ONE TENTH of their start (the margin of 30 x covers fp32, the D-SSIM term and the
    interval).  Camera 0, the gauge, is bitwise untouched."""
    tr, cams, truth = make_trainer(gpu, dict(pose_opt=True, pose_lr_rotation=1e-3, pose_lr_translation=1e-3, pose_opt_interval=interval))
    c0 = cams[0]
    keep = (c0.world_view_transform, c0.full_proj_transform, c0.camera_center)
    keep_vals = [t.clone() for t in keep] + [c0.R.copy(), c0.T.copy()]
    start = [pose_error(cams[k], truth[k]) for k in (1, 2)]
    for a, t in start:
        assert 1.2 < a < 1.3 and 0.025 < t < 0.029, start
    for _ in range(150):
        for c in cams:
            tr.train_step(c)
    torch.cuda.synchronize()
    assert tr.pose_updates == 300
    end = [pose_error(cams[k], truth[k]) for k in (1, 2)]
    print(f"interval {interval}: start {start} -> end {end}")
    measurements("pose_recovery", interval=interval, start=start, end=end)
    for (a0, t0), (a1, t1) in zip(start, end):
        assert a1 <= 0.1 * a0 and t1 <= 0.1 * t0, (start, end)
    assert all(a is b for a, b in zip((c0.world_view_transform, c0.full_proj_transform, c0.camera_center), keep))
    for a, b in zip(keep, keep_vals[:3]):
        assert torch.equal(a, b)
    assert np.array_equal(c0.R, keep_vals[3]) and np.array_equal(c0.T, keep_vals[4]) and not hasattr(c0, "pose_adam")


# ---------------------------------------------------------------------------------------------------------------- 7
def test_off_is_the_old_path(gpu, monkeypatch):
    """pose_opt = False: syn3r_raster_backward_cam is never invoked (both step routes) and the trainer holds no table; pose_opt = True
    with pose_opt_cameras = "pseudo": a step on a TRAINING camera does not invoke it either, a step on a pseudo-view does."""
    from syn3r_amd import _lib as L
    lib = L.load()
    calls = {"n": 0}
    real = lib.syn3r_raster_backward_cam

    def counting(*a):
        calls["n"] += 1
        return real(*a)

    monkeypatch.setattr(lib, "syn3r_raster_backward_cam", counting, raising=True)
    tr, cams, _ = make_trainer(gpu, {}, n=300)
    poses = [(c.R.copy(), c.T.copy(), c.world_view_transform) for c in cams]
    for explicit in (True, False):
        for c in cams:
            tr.train_step(c, explicit=explicit)
    assert calls["n"] == 0 and tr.pose.table is None and tr.pose_updates == 0
    for c, (R, T, v) in zip(cams, poses):
        assert np.array_equal(c.R, R) and np.array_equal(c.T, T) and c.world_view_transform is v
    tr, cams, truth = make_trainer(gpu, dict(pose_opt=True, pose_opt_cameras="pseudo", pose_opt_interval=1), n=300)
    tr.update_cameras([cams[2].original_image], [truth[2]], intrinsics(), 0.5)
    for explicit in (True, False):
        for c in cams:
            tr.train_step(c, explicit=explicit)
    assert calls["n"] == 0 and tr.pose_updates == 0
    pseudo = tr.pseudo_cameras[0]
    before = pseudo.world_view_transform
    tr.train_step(pseudo, explicit=True)
    tr.train_step(pseudo, explicit=False)
    assert calls["n"] == 2 and tr.pose_updates == 2 and pseudo.world_view_transform is not before


# ---------------------------------------------------------------------------------------------------------------- 8
def test_camera_list_change_applies_what_is_pending(gpu):
    """`update_cameras(append=True)` in the middle of an interval: the pending gradient moves its camera, the surviving cameras keep
    their Adam state, and the fresh table has a row for the new view."""
    tr, cams, truth = make_trainer(gpu, dict(pose_opt=True, pose_opt_interval=5), n=300)
    for _ in range(5):
        tr.train_step(cams[1])
    assert tr.pose_updates == 1 and cams[1].pose_adam["t"] == 1
    tr.train_step(cams[1])
    tr.train_step(cams[2])
    assert tr.pose.counts == [0, 1, 1] and tr.pose_updates == 1
    R1, state1 = cams[1].R.copy(), cams[1].pose_adam
    assert not hasattr(cams[2], "pose_adam")
    tr.update_cameras([cams[2].original_image], [truth[2]], intrinsics(), 0.5, append=True)
    assert tr.pose_updates == 3 and tr.pose.table is None
    assert cams[1].pose_adam is state1 and state1["t"] == 2 and cams[2].pose_adam["t"] == 1 and not np.array_equal(cams[1].R, R1)
    tr.train_step(tr.pseudo_cameras[0])
    assert tuple(tr.pose.table.shape) == (4, 35) and tr.pose.counts == [0, 0, 0, 1]
    tr.reset_gs()
    assert tr.pose_updates == 4 and tr.pose.table is None and tr.pseudo_cameras[0].pose_adam["t"] == 1


def test_checkpoint_round_trip(gpu, tmp_path):
    """save / load restores poses and Adam state bitwise and the next update is that of the uninterrupted run (to pose_lr x the
    gradient bar 2e-3 = 2e-6: the two runs' gradients differ by the order of the blend backward's float atomics, and an Adam step is at
    most ~ the rate); a checkpoint in the format of before the option (no `camera_poses` key) still loads and moves nothing."""
    from syn3r_amd.gs.pose import camera_w2c
    kw = dict(pose_opt=True, pose_opt_interval=1)
    tr, cams, _ = make_trainer(gpu, kw, n=300, tmp=str(tmp_path))
    for _ in range(4):
        tr.train_step(cams[1])
        tr.train_step(cams[2])
    path = tr.save_checkpoint(8)
    saved = [(c.R.copy(), c.T.copy(), {k: np.copy(v) for k, v in getattr(c, "pose_adam", {}).items()}) for c in cams]
    tr.train_step(cams[1])
    tr2, cams2, _ = make_trainer(gpu, kw, n=300, tmp=str(tmp_path))
    tr2.train_step(cams2[2])                     # (something pending and another pose before the load: both are replaced)
    tr2.load_checkpoint(path)
    assert tr2.iteration == 8
    for c, (R, T, st) in zip(cams2, saved):
        assert np.array_equal(c.R, R) and np.array_equal(c.T, T)
        assert torch.equal(c.world_view_transform.cpu(), torch.tensor(camera_w2c(c), dtype=torch.float32).t())
        if st:
            assert c.pose_adam["t"] == int(st["t"]) and np.array_equal(c.pose_adam["m"], st["m"]) and np.array_equal(c.pose_adam["v"], st["v"])
        else:
            assert not hasattr(c, "pose_adam")
    assert not hasattr(cams2[0], "pose_adam") and cams2[1].pose_adam["t"] == 4
    tr2.train_step(cams2[1])
    assert cams2[1].pose_adam["t"] == 5 == cams[1].pose_adam["t"]
    assert np.abs(cams2[1].R - cams[1].R).max() <= 2e-6 and np.abs(cams2[1].T - cams[1].T).max() <= 2e-6
    assert not np.array_equal(cams[1].R, saved[1][0])
    # the parent format: (capture(), iteration) without the key
    old = str(tmp_path / "old_format.pth")
    state = tr.gaussians.capture()
    assert "camera_poses" not in state
    torch.save((state, 3), old)
    before = [(c.R.copy(), c.world_view_transform) for c in cams2]
    tr2.load_checkpoint(old)
    assert tr2.iteration == 3
    for c, (R, v) in zip(cams2, before):
        assert np.array_equal(c.R, R) and c.world_view_transform is v
    # option off: the file has the keys it always had
    tr3, _, _ = make_trainer(gpu, {}, n=300, tmp=str(tmp_path))
    st3, _ = torch.load(tr3.save_checkpoint(1), weights_only=True)
    assert "camera_poses" not in st3


def test_pose_update_renews_the_filter(gpu):
    """filter_3d = True: a pose update drops the filter's camera table, so the next step computes the filter again"""
    tr, cams, _ = make_trainer(gpu, dict(pose_opt=True, pose_opt_interval=2, filter_3d=True), n=300)
    tr.train_step(cams[1])
    n0 = tr.filter_3d_computes
    tr.train_step(cams[1])                       # the update happens at the end of this step
    assert tr.filter_3d_computes == n0 and tr.pose_updates == 1 and tr.filter3d.table is None
    tr.train_step(cams[0])
    assert tr.filter_3d_computes == n0 + 1
    tr.train_step(cams[0])                       # nothing pending for an eligible camera: no update, no new filter
    tr.train_step(cams[0])
    assert tr.filter_3d_computes == n0 + 1 and tr.pose_updates == 1
