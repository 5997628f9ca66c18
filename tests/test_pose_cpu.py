"""Camera-pose refinement, host side (syn3r_amd/gs/pose.py, Camera.set_pose, the launcher flags): the exponential map against
torch's matrix exponential, the chain rule from the rasteriser's raw camera gradient to the pose tangent against autograd and
central differences of the float64 reference (tests/raster_pose_ref.py), the pose optimiser against torch.optim.Adam, and the
plumbing.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_aa_ref as A  # noqa: E402
import raster_pose_ref as P  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("theta", [0.0, 1e-9, 0.3, 3.0])
def test_se3_exp_equals_matrix_exp(theta):
    """closed form (Rodrigues + V, series for small |phi|) == torch.linalg.matrix_exp of the 4 x 4 twist, to 1e-12"""
    from syn3r_amd.gs.pose import se3_exp
    axis = np.array([0.3, -0.5, 0.8])
    xi = np.concatenate([[0.4, -1.1, 0.7], theta * axis / np.linalg.norm(axis)])
    got = se3_exp(xi)
    ref = P.exp_twist(xi).numpy()
    assert got.dtype == np.float64 and got.shape == (4, 4)
    assert np.abs(got - ref).max() <= 1e-12
    assert np.array_equal(got[3], [0.0, 0.0, 0.0, 1.0])
    if theta == 0.0:
        assert np.array_equal(got[:3, :3], np.eye(3)) and np.array_equal(got[:3, 3], xi[:3])


# ---------------------------------------------------------------------------------------------------------------- 2
def test_tangent_from_raw_equals_autograd_and_differences():
    """On the (300, 33, 50) scene from Exp(XI0): tangent_from_raw of the reference's independent (dV, dF, dc) == autograd of the same
    loss through Exp(xi) w2c at xi = 0 to 1e-10 of the largest component, and == the central difference (h = 1e-6) of the full
    re-render to 1e-6 of it (measured 1.2e-9: no discontinuity of the rasteriser lies within h on this scene)."""
    from syn3r_amd.gs.pose import tangent_from_raw
    shape = A.SHAPES[1]
    ref = P.reference(shape)
    sc = ref["sc"]
    raw = ref["raw"].numpy()
    assert raw.shape == (35,) and np.abs(raw[[3, 7, 11, 15, 18, 22, 26, 30]]).max() == 0.0          # the slots the render never reads
    assert np.abs(raw[32:]).max() > 0 and np.abs(raw[:16]).max() > 0 and np.abs(raw[16:32]).max() > 0
    got = tangent_from_raw(raw, w2c=sc["w2c"].numpy(), projection=sc["P"].numpy())
    auto = P.tangent_by_autograd(sc, ref["deg"]).numpy()
    top = np.abs(auto).max()
    print("tangent:", got, "autograd:", auto, "rel:", np.abs(got - auto).max() / top)
    assert np.abs(got - auto).max() <= 1e-10 * top
    fd = P.tangent_by_differences(sc, ref["deg"])
    print("central differences:", fd, "rel:", np.abs(got - fd).max() / top)
    assert np.abs(got - fd).max() <= 1e-6 * top


def test_tangent_from_raw_reads_a_camera():
    """the `cam` form reads R, T and projection_matrix of a Camera: the same numbers as the explicit form"""
    from syn3r_amd.gs import Camera
    from syn3r_amd.gs.pose import camera_w2c, se3_exp, tangent_from_raw
    w2c = se3_exp(P.XI0)
    cam = Camera(0, w2c[:3, :3].T, w2c[:3, 3], 1.0, 0.8, torch.rand(3, 20, 30), data_device="cpu")
    raw = np.random.default_rng(0).standard_normal(35)
    a = tangent_from_raw(raw, cam)
    b = tangent_from_raw(raw, w2c=camera_w2c(cam), projection=cam.projection_matrix.double().numpy().T)
    assert np.array_equal(a, b)
    assert np.abs(camera_w2c(cam) - w2c).max() < 1e-7


# ---------------------------------------------------------------------------------------------------------------- 3
def test_pose_optimizer_is_adam():
    """20 steps on a fixed gradient sequence: the step equals torch.optim.Adam's on a float64 6-vector (two groups: the rates of rho
    and phi; betas 0.9 / 0.999, eps 1e-15) to 1e-12"""
    from syn3r_amd.gs.pose import PoseOptimizer
    lr_r, lr_t = 2e-3, 5e-4
    popt = PoseOptimizer(lr_rotation=lr_r, lr_translation=lr_t)
    state = popt.new_state()
    rho, phi = torch.zeros(3, dtype=torch.float64, requires_grad=True), torch.zeros(3, dtype=torch.float64, requires_grad=True)
    adam = torch.optim.Adam([{"params": [rho], "lr": lr_t}, {"params": [phi], "lr": lr_r}], betas=(0.9, 0.999), eps=1e-15)
    g = torch.Generator().manual_seed(2)
    for k in range(20):
        grad = torch.randn(6, generator=g, dtype=torch.float64) * (10.0 ** (k % 5 - 2))
        before = torch.cat([rho.detach(), phi.detach()]).clone()
        rho.grad, phi.grad = grad[:3].clone(), grad[3:].clone()
        adam.step()
        ref_step = (before - torch.cat([rho.detach(), phi.detach()])).numpy()
        step = popt.step_vector(state, grad.numpy())
        assert np.abs(step - ref_step).max() <= 1e-12, (k, step, ref_step)
    assert state["t"] == 20


def test_pose_optimizer_keeps_the_rotation_orthonormal():
    """after 1000 random steps R^T R - I <= 1e-12 and det R = +1; the update is M <- Exp(-step) M"""
    from syn3r_amd.gs.pose import PoseOptimizer, se3_exp
    popt = PoseOptimizer(lr_rotation=5e-2, lr_translation=5e-2)
    state = popt.new_state()
    M = se3_exp(P.XI0)
    rng = np.random.default_rng(4)
    g0 = rng.standard_normal(6)
    s2 = popt.new_state()
    M1 = popt.update(M, s2, g0)
    step0 = PoseOptimizer(5e-2, 5e-2).step_vector(PoseOptimizer.new_state(), g0)
    assert np.abs(M1 - se3_exp(-step0) @ M).max() <= 1e-14
    for _ in range(1000):
        M = popt.update(M, state, rng.standard_normal(6))
    R = M[:3, :3]
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12
    assert abs(np.linalg.det(R) - 1.0) <= 1e-12 and np.array_equal(M[3], [0, 0, 0, 1])


# ---------------------------------------------------------------------------------------------------------------- 4
def test_camera_set_pose():
    from syn3r_amd.gs import Camera
    from syn3r_amd.gs.pose import se3_exp
    cam = Camera(0, np.eye(3), np.zeros(3), 1.0, 0.8, torch.rand(3, 20, 30), data_device="cpu")
    old = (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)
    old_vals = [t.clone() for t in old]
    proj = cam.projection_matrix
    w2c = se3_exp((0.3, -0.2, 0.5, 0.2, 0.1, -0.3))
    cam.set_pose(w2c[:3, :3].T, w2c[:3, 3])
    new = (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)
    for a, b, v in zip(old, new, old_vals):
        assert a is not b and a.data_ptr() != b.data_ptr() and torch.equal(a, v)        # new objects; the old ones untouched
    assert cam.projection_matrix is proj
    assert cam.R.dtype == np.float32 and cam.T.dtype == np.float32
    R_w2c, t = cam.R.T.astype(np.float64), cam.T.astype(np.float64)
    assert np.abs(cam.camera_center.double().numpy() - (-R_w2c.T @ t)).max() <= 1e-6
    assert torch.equal(cam.full_proj_transform, cam.world_view_transform @ cam.projection_matrix)
    K, got = cam.get_calib_matrix_nerf()
    assert np.abs(got.double().numpy() - w2c).max() <= 1e-6 and tuple(got.shape) == (4, 4)
    assert torch.equal(got, cam.world_view_transform.t())
    assert np.abs(cam.world_view_transform.inverse()[3, :3].numpy() - cam.camera_center.numpy()).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- 5
def test_launcher_flags_and_defaults():
    from syn3r_amd import launch
    from syn3r_amd.gs import OptimizationParams
    d = OptimizationParams()
    assert (d.pose_opt, d.pose_opt_cameras, d.pose_lr_rotation, d.pose_lr_translation, d.pose_opt_interval, d.pose_opt_from_iter) == \
        (False, "all", 1e-3, 1e-3, 10, 0)
    off = launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x"]))
    assert off == d
    off = launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x", "--pose_opt", "0"]))
    assert off.pose_opt is False
    on = launch.apply_trainer_flags(OptimizationParams(), launch.parse(
        ["--scenes", "x", "--pose_opt", "1", "--pose_opt_cameras", "pseudo", "--pose_lr_rotation", "2e-3", "--pose_lr_translation", "5e-4",
         "--pose_opt_interval", "4"]))
    assert (on.pose_opt, on.pose_opt_cameras, on.pose_lr_rotation, on.pose_lr_translation, on.pose_opt_interval) == \
        (True, "pseudo", 2e-3, 5e-4, 4)
    eq = launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x", "--pose_opt=1", "--pose_opt_interval=3"]))
    assert eq.pose_opt is True and eq.pose_opt_interval == 3 and eq.pose_opt_cameras == "all"
    for bad in (["--pose_opt", "2"], ["--pose_op", "1"], ["--pose_opt_cameras", "test"], ["--pose_lr_rot", "0.1"]):
        with pytest.raises(SystemExit):
            launch.parse(["--scenes", "x"] + bad)


def test_python_surface_defaults():
    """the new arguments are optional and default to off: the existing calls are untouched"""
    import inspect
    from syn3r_amd import _lib as L
    from syn3r_amd import raster
    sig = inspect.signature(raster.rasterize_backward).parameters
    assert sig["camera_grad_out"].default is None and sig["camera_grad_accumulate"].default is False
    sig = inspect.signature(raster.GaussianRasterizer.forward).parameters
    assert sig["camera_grad"].default is None and sig["camera_grad_accumulate"].default is False
    assert L.CAMERA_GRAD == 35
    assert "syn3r_raster_backward_cam" in L.SIGNATURES and "syn3r_raster_backward_cam_workspace_bytes" in L.SIGNATURES
    assert len(L.SIGNATURES["syn3r_raster_backward_cam"][1]) == len(L.SIGNATURES["syn3r_raster_backward_abs"][1]) + 2
