"""What the trainer's host objects hold and write, with the literal names the code before the split into modules used: the keys of
`GaussianModel.capture()`, the keys of a checkpoint with `pose_opt` on, a file in that format loading back, the names importable
from `syn3r_amd.gs.trainer`, and the trainer's attributes.  No GPU."""
import numpy as np
import torch

MODEL_KEYS = {"active_sh_degree", "xyz", "features", "scaling", "rotation", "opacity", "confidence"}
POSE_KEYS = {"index", "is_pseudo", "R", "T"}
ADAM_KEYS = {"m", "v", "t"}


def _trainer(tmp_path=None, n=6, **opt_kw):
    from syn3r_amd.gs import Camera, GaussianModel, GSTrainer, OptimizationParams
    g = torch.Generator().manual_seed(3)
    r = lambda *shape: torch.randn(*shape, generator=g)
    gm = GaussianModel(r(n, 3), r(n, 3), r(n, 4), r(n), r(n, 4, 3), sh_degree=1, device="cpu")
    K = np.array([[20.0, 0, 8], [0, 20.0, 6], [0, 0, 1]], dtype=np.float32)
    cams = []
    for k in range(3):
        w2c = np.eye(4, dtype=np.float32)
        w2c[0, 3] = 0.1 * k
        cams.append(Camera.from_w2c(w2c, K, 12, 16, image=torch.rand(3, 12, 16, generator=g), data_device="cpu"))
    return GSTrainer(gm, cams, OptimizationParams(iterations=5, **opt_kw), model_path=str(tmp_path) if tmp_path else None), cams


def test_capture_keys_with_and_without_the_filter():
    tr, _ = _trainer()
    gm = tr.gaussians
    assert set(gm.capture()) == MODEL_KEYS
    gm.filter_3D = torch.full((6,), 0.25)
    state = gm.capture()
    assert set(state) == MODEL_KEYS | {"filter_3D"} and torch.equal(state["filter_3D"], gm.filter_3D)
    assert state["xyz"] is not gm._xyz and torch.equal(state["xyz"], gm._xyz.detach())


def test_checkpoint_keys_with_pose_opt_and_the_file_loads_back(tmp_path):
    tr, cams = _trainer(tmp_path, pose_opt=True)
    cams[1].pose_adam = {"m": np.arange(6.0), "v": np.arange(6.0) ** 2, "t": 4}
    tr.update_cameras([torch.rand(3, 12, 16)], [np.eye(4, dtype=np.float32)], np.array([[20.0, 0, 8], [0, 20.0, 6], [0, 0, 1]]), 0.5)
    state, it = torch.load(tr.save_checkpoint(7), weights_only=True)
    assert it == 7 and set(state) == MODEL_KEYS | {"camera_poses"}
    poses = state["camera_poses"]
    assert [set(e) for e in poses] == [POSE_KEYS, POSE_KEYS | ADAM_KEYS, POSE_KEYS, POSE_KEYS]
    assert [int(e["index"]) for e in poses] == [0, 1, 2, 3] and [int(e["is_pseudo"]) for e in poses] == [0, 0, 0, 1]
    assert poses[1]["R"].dtype == torch.float32 and poses[1]["m"].dtype == torch.float64 and poses[1]["t"] == 4
    # option off: the file has the model's keys alone
    tr0, _ = _trainer(tmp_path)
    assert set(torch.load(tr0.save_checkpoint(1), weights_only=True)[0]) == MODEL_KEYS
    # a file with exactly these keys (what the code before the split wrote) loads into a fresh trainer: poses, Adam state, iteration
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)
    written = {"active_sh_degree": 1, "xyz": torch.ones(4, 3), "features": torch.zeros(4, 4, 3), "scaling": torch.zeros(4, 3),
               "rotation": torch.ones(4, 4), "opacity": torch.zeros(4), "confidence": torch.ones(4), "filter_3D": torch.full((4,), 0.5),
               "camera_poses": [{"index": 0, "is_pseudo": 0, "R": torch.eye(3), "T": torch.zeros(3)},
                                {"index": 1, "is_pseudo": 0, "R": torch.from_numpy(R), "T": torch.tensor([1.0, 2.0, 3.0]),
                                 "m": torch.arange(6.0, dtype=torch.float64), "v": torch.ones(6, dtype=torch.float64), "t": 9},
                                {"index": 3, "is_pseudo": 1, "R": torch.eye(3), "T": torch.ones(3)}]}
    path = str(tmp_path / "parent_format.pth")
    torch.save((written, 11), path)
    tr2, cams2 = _trainer(tmp_path, pose_opt=True)
    cams2[2].pose_adam = {"m": np.ones(6), "v": np.ones(6), "t": 1}
    before = cams2[2].world_view_transform
    tr2.load_checkpoint(path)
    assert tr2.iteration == 11 and tr2.gaussians._xyz.shape == (4, 3) and torch.equal(tr2.gaussians.filter_3D, written["filter_3D"])
    assert np.array_equal(cams2[1].R, R) and np.array_equal(cams2[1].T, np.array([1, 2, 3], np.float32))
    assert cams2[1].pose_adam["t"] == 9 and np.array_equal(cams2[1].pose_adam["m"], np.arange(6.0))
    assert not hasattr(cams2[0], "pose_adam")
    assert cams2[2].world_view_transform is before and cams2[2].pose_adam["t"] == 1      # (entry 3: no such camera, entry 2: none)
    assert tr2.optimizer.param_groups[0]["params"][0] is tr2.gaussians._xyz


def test_trainer_module_keeps_its_names_and_the_trainer_its_surface():
    import syn3r_amd.gs as gs
    import syn3r_amd.gs.trainer as T
    for name in ("Camera", "GaussianModel", "GSTrainer", "OptimizationParams", "expon_lr", "build_rotation", "SH_C0", "_Scene",
                 "_world2view", "_projection"):
        assert hasattr(T, name), name
    assert gs.GSTrainer is T.GSTrainer and gs.Camera is T.Camera and gs.OptimizationParams is T.OptimizationParams
    tr, cams = _trainer(pose_opt=True, filter_3d=True)
    assert not [a for a in list(vars(tr)) + dir(type(tr)) if a.startswith(("_pose_", "_f3d_"))]
    for name in ("densify_and_prune", "reset_opacity", "proximity_unpool", "ensure_filter_3D", "apply_pose_updates", "flush_pose_updates",
                 "reset_gs", "update_cameras", "training", "finetune", "train_step", "_explicit_step", "_autograd_step"):
        assert callable(getattr(tr, name)), name
    assert (tr.last_unpooled, tr.filter_3d_computes, tr.pose_updates, tr.truncated_renders) == (0, 0, 0, 0)
    assert tr.scene.train_cameras[1.0] == cams and tr.checkpoint_iterations == []
    gm = tr.gaussians
    assert gm.xyz_gradient_accum is None and gm.denom is None and gm.max_radii2D is None and gm.xyz_gradient_accum_abs is None
    gm.ensure_stats()
    assert gm.xyz_gradient_accum.shape == (6, 1) and gm.xyz_gradient_accum_abs is None
    gm.ensure_stats(True)
    assert gm.xyz_gradient_accum_abs.shape == (6, 1)
