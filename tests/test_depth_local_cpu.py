"""The patch-wise depth-correlation term without a GPU: the launcher flags, the trainer's defaults and its origin sequence, and the
argument checks of the C-ABI entries (syn3r_depth_corr_local_*), which reject a call on the host before any HIP work."""
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
MIN, A, B = 0, 1, 2
ENTRIES = ("syn3r_depth_corr_local_workspace_bytes", "syn3r_depth_corr_local_loss", "syn3r_depth_corr_local_loss_backward",
           "syn3r_depth_corr_local_loss_step")


@pytest.fixture(scope="module")
def lib():
    from syn3r_amd import _lib, build
    build.build()
    return _lib.load()


def test_launcher_flags_and_defaults():
    from syn3r_amd import launch
    a = launch.parse(["--scenes", "x", "--depth_local_weight", "0.25", "--depth_patch_size", "16"])
    assert a.depth_local_weight == 0.25 and a.depth_patch_size == 16
    assert not a.ignored_flags
    b = launch.parse(["--scenes", "x"])
    assert b.depth_local_weight == 0.0 and b.depth_patch_size == 32 and b.depth_weight == 0.0


def test_trainer_defaults_leave_the_term_off():
    from syn3r_amd.gs import OptimizationParams
    o = OptimizationParams()
    assert o.depth_local_weight == 0.0 and o.depth_patch_size == 32 and o.depth_patch_jitter is True
    assert o.depth_weight == 0.0 and o.depth_offset == 200.0


def test_header_and_signatures_list_the_entries():
    from syn3r_amd import _lib
    header = (ROOT / "include" / "syn3r_hip.h").read_text()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES[ENTRIES[0]][0] is _lib.c_sz and len(_lib.SIGNATURES[ENTRIES[0]][1]) == 5


def _err(lib):
    return lib.syn3r_last_error().decode()


def test_entries_reject_bad_arguments(lib):
    buf = (ctypes.c_char * 65536)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    aligned = (p + 255) & ~255
    H, W, P, oy, ox = 20, 30, 8, 3, 5                    # K = 2 * 3
    wsb = lib.syn3r_depth_corr_local_workspace_bytes
    need = wsb(H, W, P, oy, ox)
    assert need > 0 and need % 256 == 0 and need >= 6 * 64 and need <= 4096
    # 0 for everything the entries reject on sizes alone
    for bad in ((0, W, P, 0, 0), (H, 0, P, 0, 0), (-1, W, P, 0, 0), ((1 << 15) + 1, W, P, 0, 0), (H, (1 << 15) + 1, P, 0, 0),
                (H, W, 1, 0, 0), (H, W, 257, 0, 0), (H, W, 0, 0, 0), (H, W, P, -1, 0), (H, W, P, 0, -1), (H, W, P, P, 0), (H, W, P, 0, P),
                (7, W, P, 0, 0), (H, 7, P, 0, 0), (8, 8, 8, 1, 0), (8, 8, 8, 0, 1), (300, 300, 256, 45, 0)):
        assert wsb(*bad) == 0, bad
    assert wsb(8, 8, 8, 0, 0) > 0 and wsb(1 << 15, 1 << 15, 256, 255, 255) > 0
    ws, parts, grad, d, pr = aligned, aligned, aligned, aligned, aligned      # never dereferenced: every call below is rejected

    def value(d_=d, p_=pr, geom=(H, W, P, oy, ox), weight=1.0, offset=200.0, mode=MIN, parts_=parts, ws_=ws, wsb_=need, acc=0):
        return lib.syn3r_depth_corr_local_loss(d_, p_, *geom, weight, offset, mode, parts_, ws_, wsb_, None)

    def step(d_=d, p_=pr, geom=(H, W, P, oy, ox), weight=1.0, offset=200.0, mode=MIN, parts_=parts, ws_=ws, wsb_=need, grad_=grad, acc=0):
        return lib.syn3r_depth_corr_local_loss_step(d_, p_, *geom, weight, offset, mode, None, parts_, grad_, acc, ws_, wsb_, None)

    def bwd(d_=d, p_=pr, geom=(H, W, P, oy, ox), weight=1.0, offset=200.0, mode=MIN, parts_=parts, ws_=ws, wsb_=need, grad_=grad, acc=0):
        return lib.syn3r_depth_corr_local_loss_backward(d_, p_, *geom, weight, offset, mode, None, ws_, wsb_, grad_, acc, None)

    for call in (value, step, bwd):
        # null pointers
        assert call(d_=None) == E_INVALID and "null" in _err(lib)
        assert call(p_=None) == E_INVALID and "null" in _err(lib)
        assert call(ws_=None) == E_INVALID and "null" in _err(lib)
        # H or W outside [1, SYN3R_SIDE_MAX]
        for g in ((0, W, P, 0, 0), (H, 0, P, 0, 0), (-3, W, P, 0, 0), ((1 << 15) + 1, W, P, 0, 0), (H, (1 << 15) + 1, P, 0, 0)):
            assert call(geom=g) == E_INVALID and "H=" in _err(lib)
        # P outside [2, 256]
        for bad_p in (1, 0, -8, 257, 1 << 20):
            assert call(geom=(H, W, bad_p, 0, 0)) == E_INVALID and "P=" in _err(lib)
        # an origin outside [0, P)
        for o in ((-1, 0), (0, -1), (P, 0), (0, P), (P + 5, P + 5)):
            assert call(geom=(H, W, P) + o) == E_INVALID and "origin" in _err(lib)
        # K = 0: no full patch fits
        for g in ((7, W, P, 0, 0), (H, 7, P, 0, 0), (8, 30, P, 1, 0), (20, 12, P, 0, 5)):
            assert call(geom=g) == E_INVALID and "K=0" in _err(lib)
        # unknown branch set
        assert call(mode=3) == E_INVALID and "mode" in _err(lib)
        assert call(mode=-1) == E_INVALID and "mode" in _err(lib)
        # non-finite weight or offset
        for w in (float("nan"), float("inf"), -float("inf")):
            assert call(weight=w) == E_INVALID and "weight" in _err(lib)
            assert call(offset=w) == E_INVALID and "offset" in _err(lib)
        # misaligned or short workspace
        assert call(ws_=ws + 4) == E_INVALID and "aligned" in _err(lib)
        assert call(wsb_=need - 1) == E_WORKSPACE and "workspace" in _err(lib)
        assert call(wsb_=0) == E_WORKSPACE and "workspace" in _err(lib)
    for call in (step, bwd):
        for acc in (2, -1, 256):
            assert call(acc=acc) == E_INVALID and "accumulate" in _err(lib)
        assert call(grad_=None) == E_INVALID and "null" in _err(lib)
    for call in (value, step):
        assert call(parts_=None) == E_INVALID and "null" in _err(lib)
        assert call(parts_=parts + 4) == E_INVALID and "parts" in _err(lib)


def test_op_rejects_cpu_tensors():
    from syn3r_amd import _lib
    from syn3r_amd.gs.train_ops import depth_correlation_local_loss, depth_correlation_local_loss_step
    d, p = torch.rand(1, 8, 8), torch.rand(8, 8)
    with pytest.raises(_lib.Syn3rError):
        depth_correlation_local_loss(d, p, 1.0, 4)
    with pytest.raises(_lib.Syn3rError):
        depth_correlation_local_loss_step(d, p, 1.0, 4)


def test_float64_restatement_is_consistent():
    """The loop restatement against itself: the differentiable form's autograd gradient is the closed-form one, a single patch
    over the whole image is the global term, and pixels in no full patch have a zero gradient."""
    from tests import depth_local_ref as R
    g = torch.Generator().manual_seed(0)
    p = torch.rand(21, 30, generator=g, dtype=torch.float64) * 5.0
    d = 4.0 - 0.3 * p + torch.rand(21, 30, generator=g, dtype=torch.float64) * 2.0
    ref = R.ref_local(d, p, 0.7, 8, (3, 5))
    assert ref["K"] == 2 * 3
    x = d.clone().requires_grad_(True)
    loss = R.ref_local_torch(x, p, 0.7, 8, (3, 5))
    loss.backward()
    assert abs(float(loss) - ref["loss"]) < 1e-14
    assert float((x.grad - ref["grad"]).abs().max()) < 1e-14
    inside = R.patch_of(21, 30, 8, 3, 5) >= 0
    assert int(inside.sum()) == 6 * 64 and not ref["grad"][~inside].any() and ref["grad"][inside].abs().min() > 0
    # one patch = the global Pearson term
    q = p[:16, :16]
    e = d[:16, :16]
    one = R.ref_local(e, q, 1.0, 16)
    ec, qc = e - e.mean(), -(q - q.mean())
    r = float((ec * qc).sum() / torch.sqrt((ec * ec).sum() * (qc * qc).sum()))
    u = 1.0 / (q + 200.0)
    uc = u - u.mean()
    rb = float((ec * uc).sum() / torch.sqrt((ec * ec).sum() * (uc * uc).sum()))
    assert abs(one["loss"] - min(1.0 - r, 1.0 - rb)) < 1e-14


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


def test_origin_sequence():
    H, W, P = 33, 50, 32
    on = dict(depth_local_weight=0.5, depth_patch_size=P)
    a, cams = _cpu_trainer(3, **on)
    b, _ = _cpu_trainer(3, **on)
    c, _ = _cpu_trainer(4, **on)
    seq = lambda tr: [tr.depth_patch_origin(cams[0], it) for it in range(200)]
    sa, sb, sc = seq(a), seq(b), seq(c)
    assert sa == sb and sa != sc
    # every origin leaves at least one full patch: oy in [0, min(P, H - P + 1)) = {0, 1}, ox in [0, 19)
    for oy, ox in sa + sc:
        assert 0 <= oy < min(P, H - P + 1) and 0 <= ox < min(P, W - P + 1)
        assert ((H - oy) // P) * ((W - ox) // P) >= 1
    assert {o[0] for o in sa} == {0, 1} and len({o[1] for o in sa}) > 10
    # a function of (seed, iteration) alone: the default is the trainer's own counter, and asking changes nothing
    a.iteration = 17
    assert a.depth_patch_origin(cams[0]) == sa[17] == a.depth_patch_origin(cams[0])
    # without jitter the origin stays at (0, 0)
    fixed, _ = _cpu_trainer(3, depth_patch_jitter=False, **on)
    assert {fixed.depth_patch_origin(cams[0], it) for it in range(20)} == {(0, 0)}
    # a camera smaller than the patch on a side is an error that names the option
    small, cams_small = _cpu_trainer(3, H=20, W=50, **on)
    with pytest.raises(ValueError, match="depth_patch_size"):
        small.depth_patch_origin(cams_small[0])


def test_camera_pick_sequence_does_not_move():
    off, _ = _cpu_trainer(7)
    on, _ = _cpu_trainer(7, depth_local_weight=0.5, depth_patch_size=32)
    picks_off, picks_on = [], []
    for it in range(100):
        picks_off.append(off.scene.getTrainCameras().index(off._pick_camera()))
        on.iteration = it
        on.depth_patch_origin(on.scene.getTrainCameras()[0])          # what a step with the term on draws
        picks_on.append(on.scene.getTrainCameras().index(on._pick_camera()))
    assert picks_off == picks_on and len(set(picks_off)) > 1
