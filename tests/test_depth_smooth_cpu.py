"""The edge-aware depth-smoothness term without a GPU: the launcher flags, the trainer's defaults and its camera picks, the float64
restatement against itself, and the argument checks of the C-ABI entries (syn3r_depth_edge_weights, syn3r_depth_smooth_*), which
reject a call on the host before any HIP work."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

E_INVALID, E_WORKSPACE = -1, -2
ENTRIES = ("syn3r_depth_edge_weights", "syn3r_depth_smooth_workspace_bytes", "syn3r_depth_smooth_loss",
           "syn3r_depth_smooth_loss_backward", "syn3r_depth_smooth_loss_step")
SIDE_MAX = 1 << 15


@pytest.fixture(scope="module")
def lib():
    from syn3r_amd import _lib, build
    build.build()
    return _lib.load()


def test_launcher_flags_and_defaults():
    from syn3r_amd import launch
    from syn3r_amd.gs import OptimizationParams
    a = launch.parse(["--scenes", "x", "--depth_smooth_weight", "0.25", "--depth_smooth_gamma", "2.5", "--depth_smooth_cameras", "pseudo"])
    assert a.depth_smooth_weight == 0.25 and a.depth_smooth_gamma == 2.5 and a.depth_smooth_cameras == "pseudo"
    assert not a.ignored_flags
    o = launch.apply_trainer_flags(OptimizationParams(), a)
    assert o.depth_smooth_weight == 0.25 and o.depth_smooth_gamma == 2.5 and o.depth_smooth_cameras == "pseudo"
    b = launch.parse(["--scenes", "x"])
    assert b.depth_smooth_weight == 0.0 and b.depth_smooth_gamma == 1.0 and b.depth_smooth_cameras == "all"
    assert launch.apply_trainer_flags(OptimizationParams(), b) == OptimizationParams()
    with pytest.raises(SystemExit):
        launch.parse(["--scenes", "x", "--depth_smooth_cameras", "test"])
    with pytest.raises(SystemExit):                                   # the trainer's flags are not abbreviated
        launch.parse(["--scenes", "x", "--depth_smooth", "0.5"])


def test_trainer_defaults_leave_the_term_off():
    from syn3r_amd.gs import OptimizationParams
    o = OptimizationParams()
    assert o.depth_smooth_weight == 0.0 and o.depth_smooth_gamma == 1.0 and o.depth_smooth_cameras == "all"
    assert o.depth_weight == 0.0 and o.depth_local_weight == 0.0


def test_header_and_signatures_list_the_entries():
    from syn3r_amd import _lib, build
    header = (ROOT / "include" / "syn3r_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES[ENTRIES[1]][0] is _lib.c_sz and len(_lib.SIGNATURES[ENTRIES[1]][1]) == 2
    assert "depth_smooth.hip" in build.STRICT_FP and (ROOT / "syn3r_amd" / "csrc" / "depth_smooth.hip").exists()
    assert "UNPINNED" in header[header.index("syn3r_depth_edge_weights") - 4000:header.index("syn3r_depth_edge_weights")]


def _err(lib):
    return lib.syn3r_last_error().decode()


def test_entries_reject_bad_arguments(lib):
    buf = (ctypes.c_char * (1 << 20))()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    base = (p + 255) & ~255
    H, W = 20, 30
    plane = H * W * 4
    # never dereferenced: every call below is rejected.  Disjoint regions: depth, weights [2 planes], grad, image [3 planes], ws, parts
    d, wgt, grad, img = base, base + 4096, base + 4096 * 4, base + 4096 * 8
    ws, parts = base + 4096 * 16, base + 4096 * 17
    assert plane <= 4096 and 3 * plane <= 4096 * 8
    wsb = lib.syn3r_depth_smooth_workspace_bytes
    need = wsb(H, W)
    assert need > 0 and need % 256 == 0 and need <= 4096
    for bad in ((0, W), (H, 0), (-1, W), (H, -7), (SIDE_MAX + 1, W), (H, SIDE_MAX + 1), (1 << 30, 1 << 30)):
        assert wsb(*bad) == 0, bad
    assert wsb(1, 1) > 0 and wsb(SIDE_MAX, SIDE_MAX) > 0 and wsb(SIDE_MAX, SIDE_MAX) <= 1 << 16

    def value(d_=d, w_=wgt, hw=(H, W), weight=1.0, parts_=parts, ws_=ws, wsb_=need, grad_=grad, acc=0):
        return lib.syn3r_depth_smooth_loss(d_, w_, *hw, weight, parts_, ws_, wsb_, None)

    def step(d_=d, w_=wgt, hw=(H, W), weight=1.0, parts_=parts, ws_=ws, wsb_=need, grad_=grad, acc=0):
        return lib.syn3r_depth_smooth_loss_step(d_, w_, *hw, weight, None, parts_, grad_, acc, ws_, wsb_, None)

    def bwd(d_=d, w_=wgt, hw=(H, W), weight=1.0, parts_=parts, ws_=ws, wsb_=need, grad_=grad, acc=0):
        return lib.syn3r_depth_smooth_loss_backward(d_, w_, *hw, weight, None, ws_, wsb_, grad_, acc, None)

    for call in (value, step, bwd):
        assert call(d_=None) == E_INVALID and "null" in _err(lib)
        assert call(w_=None) == E_INVALID and "null" in _err(lib)
        assert call(ws_=None) == E_INVALID and "null" in _err(lib)
        for hw in ((0, W), (H, 0), (-3, W), (H, -3), (SIDE_MAX + 1, W), (H, SIDE_MAX + 1), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert call(hw=hw) == E_INVALID and "H=" in _err(lib)
        for w in (float("nan"), float("inf"), -float("inf")):
            assert call(weight=w) == E_INVALID and "weight" in _err(lib)
        assert call(ws_=ws + 4) == E_INVALID and "aligned" in _err(lib)
        assert call(wsb_=need - 1) == E_WORKSPACE and "workspace" in _err(lib)
        assert call(wsb_=0) == E_WORKSPACE and "workspace" in _err(lib)
    for call in (step, bwd):
        for acc in (2, -1, 256):
            assert call(acc=acc) == E_INVALID and "accumulate" in _err(lib)
        assert call(grad_=None) == E_INVALID and "null" in _err(lib)
        # grad_depth over the depth, over either weight plane, one byte into one
        for g in (d, d + 4, d + plane - 4, d - plane + 4, wgt, wgt + plane, wgt + 2 * plane - 4, wgt - plane + 4):
            assert call(grad_=g) == E_INVALID and "aliases" in _err(lib), g - base
    for call in (value, step):
        assert call(parts_=None) == E_INVALID and "null" in _err(lib)
        assert call(parts_=parts + 4) == E_INVALID and "parts" in _err(lib)

    def weights(img_=img, hw=(H, W), gamma=1.0, out_=wgt):
        return lib.syn3r_depth_edge_weights(img_, *hw, gamma, out_, None)

    assert weights(img_=None) == E_INVALID and "null" in _err(lib)
    assert weights(out_=None) == E_INVALID and "null" in _err(lib)
    for hw in ((0, W), (H, 0), (-3, W), (SIDE_MAX + 1, W), (H, SIDE_MAX + 1)):
        assert weights(hw=hw) == E_INVALID and "H=" in _err(lib)
    for g in (float("nan"), float("inf"), -float("inf"), -1.0, -1e-30):
        assert weights(gamma=g) == E_INVALID and "gamma" in _err(lib)
    for o in (img, img + 4, img + 3 * plane - 4, img - 2 * plane + 4):
        assert weights(out_=o) == E_INVALID and "aliases" in _err(lib)


def test_op_rejects_cpu_tensors():
    from syn3r_amd import _lib
    from syn3r_amd.gs.train_ops import depth_edge_weights, depth_smoothness_loss, depth_smoothness_loss_step
    d, w, img = torch.rand(1, 8, 8), torch.rand(2, 8, 8), torch.rand(3, 8, 8)
    with pytest.raises(_lib.Syn3rError):
        depth_edge_weights(img)
    with pytest.raises(_lib.Syn3rError):
        depth_smoothness_loss(d, w)
    with pytest.raises(_lib.Syn3rError):
        depth_smoothness_loss_step(d, w)


def _case(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    d = 0.5 + 5.5 * torch.rand(H, W, generator=g, dtype=torch.float64)
    w = torch.rand(2, H, W, generator=g, dtype=torch.float64)
    return d, w


def test_float64_restatement_is_consistent():
    """The closed-form gradient is autograd of the formula to 1e-14, ties included; W == 1, H == 1, 1 x 1 and m <= 0 behave as
    specified; the last column of wx and the last row of wy are never read."""
    from tests import depth_smooth_ref as R
    for H, W in ((21, 30), (3, 5), (2, 2), (1, 7), (7, 1), (1, 1)):
        d, w = _case(H, W, H * 100 + W)
        if H > 2 and W > 3:
            d[1, 2] = d[1, 1]                                           # ties: sign(0) = 0 in both
            d[2, 0] = d[1, 0]
        ref = R.ref_smooth(d, w, 0.7, grad_loss=1.3)
        x = d.clone().requires_grad_(True)
        loss = R.ref_smooth_torch(x, w, 0.7)
        (loss * 1.3).backward()
        assert abs(float(loss) - ref["loss"]) <= 1e-14 * max(1.0, abs(ref["loss"]))
        assert float((x.grad - ref["grad"]).abs().max()) <= 1e-14
        assert abs(ref["m"] - float(d.mean())) <= 1e-15
        if W == 1:
            assert ref["sx"] == 0.0
        if H == 1:
            assert ref["sy"] == 0.0
        if H == 1 and W == 1:
            assert ref["loss"] == 0.0 and float(ref["grad"]) == 0.0
        elif min(H, W) > 1:
            assert ref["loss"] > 0.0 and ref["sx"] > 0.0 and ref["sy"] > 0.0
        # the gradient of a scale-invariant loss is orthogonal to d: sum_i d_i grad_i = 0
        assert abs(float((d * ref["grad"]).sum())) <= 1e-13
        # the absent column and row
        w2 = w.clone()
        w2[0, :, -1] = float("nan")
        w2[1, -1, :] = float("inf")
        other = R.ref_smooth(d, w2, 0.7, grad_loss=1.3)
        assert other["loss"] == ref["loss"] and torch.equal(other["grad"], ref["grad"])
    # an empty render: zero loss, zero gradient, no NaN
    d, w = _case(5, 6, 1)
    for empty in (torch.zeros_like(d), -d):
        ref = R.ref_smooth(empty, w, 1.0)
        assert ref["loss"] == 0.0 and not ref["grad"].any() and ref["empty"]
        x = empty.clone().requires_grad_(True)
        R.ref_smooth_torch(x, w, 1.0).backward()
        assert not x.grad.any()
    # the weights: exp(-gamma mean_c |difference|), zeros where no pair exists
    img = torch.rand(3, 4, 5, generator=torch.Generator().manual_seed(3))
    ew = R.ref_weights(img, 2.0)
    assert not ew[0, :, -1].any() and not ew[1, -1, :].any()
    i64 = img.double()
    assert abs(float(ew[0, 1, 2]) - float(torch.exp(-2.0 * (i64[:, 1, 3] - i64[:, 1, 2]).abs().mean()))) <= 1e-15
    assert abs(float(ew[1, 2, 4]) - float(torch.exp(-2.0 * (i64[:, 3, 4] - i64[:, 2, 4]).abs().mean()))) <= 1e-15
    assert float(R.ref_weights(torch.zeros(3, 4, 5), 1.0)[0, :, :-1].min()) == 1.0


def _cpu_trainer(seed, H=33, W=50, n_cams=5, **opt_kw):
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    from syn3r_amd.gs.gaussian_model import GaussianModel
    g = torch.Generator().manual_seed(0)
    r = lambda *shape: torch.randn(*shape, generator=g)
    gm = GaussianModel(r(6, 3), r(6, 3), r(6, 4), r(6), r(6, 4, 3), sh_degree=1, device="cpu")
    K = np.array([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1]], dtype=np.float32)
    cams = []
    for k in range(n_cams):
        w2c = np.eye(4, dtype=np.float32)
        w2c[0, 3] = 0.1 * k
        cams.append(Camera.from_w2c(w2c, K, H, W, image=torch.rand(3, H, W, generator=g), data_device="cpu"))
    return GSTrainer(gm, cams, OptimizationParams(iterations=5, seed=seed, **opt_kw)), cams


def test_camera_pick_sequence_does_not_move():
    off, _ = _cpu_trainer(7)
    on, _ = _cpu_trainer(7, depth_smooth_weight=0.5, depth_smooth_cameras="train")
    picks = lambda tr: [tr.scene.getTrainCameras().index(tr._pick_camera()) for _ in range(100)]
    a, b = picks(off), picks(on)
    assert a == b and len(set(a)) > 1


def test_unknown_camera_kind_and_camera_planes():
    from syn3r_amd.gs import Camera
    with pytest.raises(ValueError, match="depth_smooth_cameras"):
        _cpu_trainer(1, depth_smooth_cameras="test")
    tr, cams = _cpu_trainer(1)
    tr.opt.depth_smooth_weight, tr.opt.depth_smooth_cameras = 0.5, "none"
    with pytest.raises(ValueError, match="depth_smooth_cameras"):
        tr._depth_smooth_weights(cams[0])
    # the term off: nothing is asked of the camera
    tr.opt.depth_smooth_weight, tr.opt.depth_smooth_cameras = 0.0, "all"
    assert tr._depth_smooth_weights(cams[0]) is None and cams[0]._depth_edge_cache is None
    # which cameras the option names (a camera's own planes: no kernel, so this runs without a GPU)
    H, W = 33, 50
    own = torch.rand(2, H, W)
    for c in cams:
        c.depth_edge_weights = own
    cams[1].is_pseudo = True
    tr.opt.depth_smooth_weight = 0.5
    for kind, want in (("all", (True, True)), ("train", (True, False)), ("pseudo", (False, True))):
        tr.opt.depth_smooth_cameras = kind
        got = tuple(tr._depth_smooth_weights(c) is not None for c in cams[:2])
        assert got == want, kind
    assert torch.equal(tr.depth_edge_weights(cams[0]), own) and cams[0]._depth_edge_cache is None
    # a camera's own planes: shape checked, [2,H,W] fp32
    K = np.array([[40.0, 0, W / 2], [0, 40.0, H / 2], [0, 0, 1]], dtype=np.float32)
    cam = Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, image=torch.rand(3, H, W), data_device="cpu",
                          depth_edge_weights=own.double())
    assert cam.depth_edge_weights.dtype == torch.float32 and cam.depth_edge_weights.shape == (2, H, W)
    with pytest.raises(ValueError, match="depth_edge_weights"):
        Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, image=torch.rand(3, H, W), data_device="cpu",
                        depth_edge_weights=torch.rand(2, H, W + 1))
    # a camera without a target image is skipped
    blank = Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, data_device="cpu")
    tr.opt.depth_smooth_cameras = "all"
    assert tr._depth_smooth_weights(blank) is None
