"""Per-camera affine exposure compensation (`OptimizationParams.exposure_opt`), the parts that need no GPU: the ABI declarations, the
option fields and launcher flags, the refusal of CPU tensors, the checkpoint format, and the float64 reference of the GPU tests
(tests/exposure_ref.py) against itself."""
import dataclasses
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import exposure_ref as R  # noqa: E402
from test_trainer_state_cpu import MODEL_KEYS, _trainer  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("syn3r_exposure_apply", "syn3r_exposure_backward_workspace_bytes", "syn3r_exposure_backward")
EXPOSURE_KEYS = {"index", "is_pseudo", "A", "m", "v", "t"}
K = np.array([[20.0, 0, 8], [0, 20.0, 6], [0, 0, 1]])


def test_reference_closed_form_equals_autograd():
    g = torch.Generator().manual_seed(5)
    for H, W in ((1, 1), (5, 7), (33, 50)):
        image = torch.randn(3, H, W, generator=g, dtype=torch.float64)
        A = torch.rand(12, generator=g, dtype=torch.float64) * 3.0 - 1.5
        grad_out = torch.randn(3, H, W, generator=g, dtype=torch.float64)
        gi, ga = R.backward(image, A, grad_out)
        gi2, ga2 = R.backward_autograd(image, A, grad_out)
        assert float((gi - gi2).abs().max()) <= 1e-12 and float((ga - ga2).abs().max()) <= 1e-12
        assert torch.equal(R.apply(image, R.IDENTITY), image)
        assert bool((R.grad_A_abs(image, grad_out) >= ga.abs()).all())


def test_header_declares_the_entries_and_the_binding_has_them():
    from syn3r_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "syn3r_hip.h").read_text(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in L.SIGNATURES, name
    assert L.SIGNATURES["syn3r_exposure_apply"] == (L.c_i, [L.c_p, L.c_p, L.c_i, L.c_i, L.c_p, L.c_p])
    assert L.SIGNATURES["syn3r_exposure_backward_workspace_bytes"] == (L.c_sz, [L.c_i, L.c_i])
    assert L.SIGNATURES["syn3r_exposure_backward"] == (L.c_i, [L.c_p, L.c_p, L.c_p, L.c_i, L.c_i, L.c_p, L.c_p, L.c_i, L.c_p, L.c_sz, L.c_p])


def test_entries_reject_bad_arguments_before_any_launch():
    """null pointers, non-positive and absurd sizes, a short workspace, an output that aliases an input: a status and a message"""
    import ctypes as C
    from syn3r_amd import _lib as L
    lib = L.load()
    buf = (C.c_float * 8192)()
    base = (C.addressof(buf) + 255) & ~255
    image, out, grad_out, A, grad_A, ws = base, base + 1024, base + 2048, base + 4096, base + 4096 + 64, base + 8192
    err = lambda: lib.syn3r_last_error().decode()
    assert lib.syn3r_exposure_apply(None, A, 4, 4, out, None) == -1 and "null" in err()
    assert lib.syn3r_exposure_apply(image, A, 0, 4, out, None) == -1 and lib.syn3r_exposure_apply(image, A, 4, -1, out, None) == -1
    assert lib.syn3r_exposure_apply(image, A, 2 ** 31 - 1, 2 ** 31 - 1, out, None) == -1
    assert lib.syn3r_exposure_apply(image, A, 4, 4, image + 16, None) == -1 and "alias" in err()
    assert lib.syn3r_exposure_apply(image, A, 1, 3, A + 8, None) == -1 and "alias" in err()
    assert lib.syn3r_exposure_backward_workspace_bytes(0, 4) == 0 and lib.syn3r_exposure_backward_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1) == 0
    need = lib.syn3r_exposure_backward_workspace_bytes(4, 4)
    assert need >= 12 * 4 and need % 256 == 0
    # the grid, and with it the workspace, is capped: 2048 blocks x 12 floats at most
    assert lib.syn3r_exposure_backward_workspace_bytes(1100, 1920) == 2048 * 12 * 4 == lib.syn3r_exposure_backward_workspace_bytes(2 ** 15, 2 ** 15)
    assert lib.syn3r_exposure_backward(image, A, grad_out, 4, 4, out, None, 0, ws, need, None) == -1 and "null" in err()
    assert lib.syn3r_exposure_backward(image, A, grad_out, 4, 4, out, grad_A, 0, ws, need - 1, None) == -2 and "workspace" in err()
    assert lib.syn3r_exposure_backward(image, A, grad_out, -4, 4, out, grad_A, 0, ws, need, None) == -1
    assert lib.syn3r_exposure_backward(image, A, grad_out, 4, 4, grad_out + 4, grad_A, 0, ws, need, None) == -1 and "alias" in err()
    assert lib.syn3r_exposure_backward(image, A, grad_out, 4, 4, image, grad_A, 0, ws, need, None) == -1 and "alias" in err()


def test_fields_defaults_and_launcher_flags():
    from syn3r_amd import launch
    from syn3r_amd.gs import OptimizationParams
    d = OptimizationParams()
    assert (d.exposure_opt, d.exposure_cameras, d.exposure_lr, d.exposure_lr_final, d.exposure_lr_max_steps) == \
        (False, "pseudo", 0.01, None, 30_000)
    base = OptimizationParams(iterations=77, lambda_dssim=0.3, seed=4)
    assert launch.apply_trainer_flags(base, launch.parse(["--scenes", "x"])) == base
    assert launch.apply_trainer_flags(base, launch.parse(["--scenes", "x", "--exposure_opt", "0"])) == base
    on = launch.apply_trainer_flags(base, launch.parse(["--scenes", "x", "--exposure_opt", "1"]))
    changed = {f.name for f in dataclasses.fields(base) if getattr(on, f.name) != getattr(base, f.name)}
    assert changed == {"exposure_opt"} and on.exposure_opt is True
    full = launch.apply_trainer_flags(base, launch.parse(["--scenes", "x", "--exposure_opt=1", "--exposure_cameras", "all", "--exposure_lr",
                                                           "2e-3", "--exposure_lr_final", "1e-4"]))
    assert (full.exposure_opt, full.exposure_cameras, full.exposure_lr, full.exposure_lr_final, full.exposure_lr_max_steps) == \
        (True, "all", 2e-3, 1e-4, 30_000)
    for bad in (["--exposure_opt", "2"], ["--exposure_op", "1"], ["--exposure_cameras", "test"], ["--exposure_lr_fin", "0.1"],
                ["--exposure", "1"]):
        with pytest.raises(SystemExit):
            launch.parse(["--scenes", "x"] + bad)


def test_bad_exposure_cameras_raises():
    with pytest.raises(ValueError, match="exposure_cameras"):
        _trainer(exposure_cameras="test")
    with pytest.raises(ValueError, match="exposure_cameras"):
        _trainer(exposure_opt=True, exposure_cameras="")


def test_cpu_tensors_are_refused():
    from syn3r_amd import _lib as L
    from syn3r_amd.gs import train_ops as T
    image, A = torch.rand(3, 4, 6), R.IDENTITY.float()
    with pytest.raises(L.Syn3rError):
        T.exposure_apply_step(image, A)
    with pytest.raises(L.Syn3rError):
        T.exposure_apply(image.requires_grad_(True), A.clone().requires_grad_(True))
    with pytest.raises(L.Syn3rError):
        T.exposure_backward_step(image.detach(), A, torch.rand(3, 4, 6), torch.zeros(12))
    tr, cams = _trainer(exposure_opt=True)
    cams[1].exposure = A.clone()
    with pytest.raises(L.Syn3rError):
        tr.exposed(image.detach(), cams[1])
    assert tr.exposed(image, cams[0]) is image


def test_lr_schedule_and_eligibility():
    from syn3r_amd.gs import OptimizationParams
    from syn3r_amd.gs.params import expon_lr
    tr, cams = _trainer(exposure_opt=True, exposure_lr=0.02)
    assert tr.exposure.lr() == 0.02
    tr.opt = OptimizationParams(exposure_opt=True, exposure_lr=0.01, exposure_lr_final=0.001, exposure_lr_max_steps=100)   # (read when needed)
    tr.iteration = 49
    assert tr.exposure.lr() == expon_lr(50, 0.01, 0.001, max_steps=100) and 0.001 < tr.exposure.lr() < 0.01
    tr.update_cameras([torch.rand(3, 12, 16)], [np.eye(4, dtype=np.float32)], K, 0.5)
    pseudo = tr.pseudo_cameras[0]
    kinds = {"pseudo": [False, False, False, True], "train": [False, True, True, False], "all": [False, True, True, True]}
    for kind, expect in kinds.items():
        tr.opt = OptimizationParams(exposure_opt=True, exposure_cameras=kind)
        assert [tr.exposure.eligible(c) for c in cams + [pseudo]] == expect, kind
    tr.opt = OptimizationParams(exposure_cameras="all")
    assert not any(tr.exposure.eligible(c) for c in cams + [pseudo]) and tr.exposure.state(pseudo) is None
    assert tr.exposure_updates == 0 and not [a for a in list(vars(tr)) + dir(type(tr)) if a.startswith(("_pose_", "_f3d_"))]


def test_checkpoint_keys_and_a_hand_written_file_loads_back(tmp_path):
    # option off: no camera has an exposure after construction, the file has the model's keys alone
    tr0, cams0 = _trainer(tmp_path)
    assert not any(hasattr(c, "exposure") or hasattr(c, "exposure_adam") for c in cams0)
    assert set(torch.load(tr0.save_checkpoint(1), weights_only=True)[0]) == MODEL_KEYS
    # option on: one entry per camera that has state, exactly the six keys
    tr, cams = _trainer(tmp_path, exposure_opt=True, exposure_cameras="all")
    assert not any(hasattr(c, "exposure") for c in cams)
    tr.update_cameras([torch.rand(3, 12, 16)], [np.eye(4, dtype=np.float32)], K, 0.5)
    pseudo = tr.pseudo_cameras[0]
    for cam, t in ((cams[2], 3), (pseudo, 8)):
        cam.exposure = torch.arange(12.0) + t
        cam.exposure_adam = {"m": torch.full((12,), 0.5 * t), "v": torch.full((12,), 0.25 * t), "t": t}
    state, it = torch.load(tr.save_checkpoint(7), weights_only=True)
    assert it == 7 and set(state) == MODEL_KEYS | {"camera_exposures"}
    entries = state["camera_exposures"]
    assert [set(e) for e in entries] == [EXPOSURE_KEYS, EXPOSURE_KEYS]
    assert [(int(e["index"]), int(e["is_pseudo"]), int(e["t"])) for e in entries] == [(2, 0, 3), (3, 1, 8)]
    assert entries[0]["A"].dtype == torch.float32 and entries[0]["A"].shape == (12,) and torch.equal(entries[1]["A"], torch.arange(12.0) + 8)
    # a hand-written file in that format loads back onto the cameras registered at those indices (of the same kind)
    written = {"active_sh_degree": 1, "xyz": torch.ones(4, 3), "features": torch.zeros(4, 4, 3), "scaling": torch.zeros(4, 3),
               "rotation": torch.ones(4, 4), "opacity": torch.zeros(4), "confidence": torch.ones(4),
               "camera_exposures": [{"index": 1, "is_pseudo": 0, "A": torch.arange(12.0), "m": torch.ones(12), "v": torch.full((12,), 2.0), "t": 9},
                                    {"index": 2, "is_pseudo": 1, "A": torch.zeros(12), "m": torch.zeros(12), "v": torch.zeros(12), "t": 1},
                                    {"index": 5, "is_pseudo": 0, "A": torch.zeros(12), "m": torch.zeros(12), "v": torch.zeros(12), "t": 1}]}
    path = str(tmp_path / "hand_written.pth")
    torch.save((written, 11), path)
    tr2, cams2 = _trainer(tmp_path, exposure_opt=True)
    tr2.load_checkpoint(path)
    assert tr2.iteration == 11 and tr2.gaussians._xyz.shape == (4, 3)
    assert torch.equal(cams2[1].exposure, torch.arange(12.0)) and cams2[1].exposure.dtype == torch.float32
    st = cams2[1].exposure_adam
    assert set(st) == {"m", "v", "t"} and st["t"] == 9 and torch.equal(st["m"], torch.ones(12)) and torch.equal(st["v"], torch.full((12,), 2.0))
    assert not hasattr(cams2[0], "exposure") and not hasattr(cams2[2], "exposure")      # (entry 2: another kind; entry 5: no such camera)
    # a trainer with the option off ignores the key; a file without the key loads as before
    tr3, cams3 = _trainer(tmp_path)
    tr3.load_checkpoint(path)
    assert tr3.iteration == 11 and not any(hasattr(c, "exposure") for c in cams3)
    tr2.load_checkpoint(tr0.save_checkpoint(2))
    assert tr2.iteration == 2 and cams2[1].exposure_adam["t"] == 9
