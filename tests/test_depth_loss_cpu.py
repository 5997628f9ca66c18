"""FSGS' depth-correlation term without a GPU: the launcher flag and the argument checks of the C-ABI entries
(syn3r_depth_corr_loss*), which reject a call on the host before any HIP work."""
import ctypes
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

E_INVALID, E_WORKSPACE = -1, -2
MIN, A, B = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from syn3r_amd import _lib, build
    build.build()
    return _lib.load()


def test_launcher_honours_depth_weight():
    from syn3r_amd import launch
    a = launch.parse(["--scenes", "x", "--depth_weight", "0.05"])
    assert a.depth_weight == 0.05
    assert "--depth_weight" not in a.ignored_flags and "0.05" not in a.ignored_flags
    assert launch.parse(["--scenes", "x"]).depth_weight == 0.0
    # FSGS' pseudo-view depth term stays tolerated and ignored
    b = launch.parse(["--scenes", "x", "--depth_weight", "0.05", "--depth_pseudo_weight", "0.5"])
    assert b.ignored_flags == ["--depth_pseudo_weight", "0.5"]


def test_trainer_defaults_leave_the_term_off():
    from syn3r_amd.gs import OptimizationParams
    o = OptimizationParams()
    assert o.depth_weight == 0.0 and o.depth_offset == 200.0


def _err(lib):
    return lib.syn3r_last_error().decode()


def test_entries_reject_bad_arguments(lib):
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    aligned = (p + 255) & ~255
    n = 64
    need = lib.syn3r_depth_corr_loss_workspace_bytes(n)
    assert need > 0 and need % 256 == 0 and need <= 2048
    assert lib.syn3r_depth_corr_loss_workspace_bytes(1) == 0
    assert lib.syn3r_depth_corr_loss_workspace_bytes(0) == 0
    assert lib.syn3r_depth_corr_loss_workspace_bytes((1 << 30) + 1) == 0
    ws, parts, grad, d, pr = aligned, aligned, aligned, aligned, aligned     # never dereferenced: every call below is rejected

    def value(d_, p_, n_, mode=MIN, ws_=ws, wsb=need, parts_=parts, offset=200.0):
        return lib.syn3r_depth_corr_loss(d_, p_, n_, 1.0, offset, mode, parts_, ws_, wsb, None)

    def step(d_, p_, n_, mode=MIN, ws_=ws, wsb=need, parts_=parts, grad_=grad):
        return lib.syn3r_depth_corr_loss_step(d_, p_, n_, 1.0, 200.0, mode, None, parts_, grad_, ws_, wsb, None)

    def bwd(d_, p_, n_, mode=MIN, ws_=ws, wsb=need, grad_=grad):
        return lib.syn3r_depth_corr_loss_backward(d_, p_, n_, 1.0, 200.0, mode, None, ws_, wsb, grad_, None)

    for call in (value, step, bwd):
        # null pointers
        assert call(None, pr, n) == E_INVALID and "null" in _err(lib)
        assert call(d, None, n) == E_INVALID and "null" in _err(lib)
        assert call(d, pr, n, ws_=None) == E_INVALID and "null" in _err(lib)
        # n < 2 (a correlation of one value is undefined), and beyond the size limit
        for bad_n in (1, 0, -5, (1 << 30) + 1):
            assert call(d, pr, bad_n) == E_INVALID and "n=" in _err(lib)
        # unknown branch set
        assert call(d, pr, n, mode=3) == E_INVALID and "mode" in _err(lib)
        # short workspace
        assert call(d, pr, n, wsb=need - 1) == E_WORKSPACE and "workspace" in _err(lib)
    assert value(d, pr, n, parts_=None) == E_INVALID and "null" in _err(lib)
    assert step(d, pr, n, grad_=None) == E_INVALID and "null" in _err(lib)
    assert step(d, pr, n, parts_=None) == E_INVALID and "null" in _err(lib)
    assert bwd(d, pr, n, grad_=None) == E_INVALID and "null" in _err(lib)
    assert value(d, pr, n, offset=float("nan")) == E_INVALID and "offset" in _err(lib)


def test_op_rejects_cpu_tensors():
    import torch
    from syn3r_amd import _lib
    from syn3r_amd.gs.train_ops import depth_correlation_loss, depth_correlation_loss_step
    d, p = torch.rand(1, 8, 8), torch.rand(8, 8)
    with pytest.raises(_lib.Syn3rError):
        depth_correlation_loss(d, p)
    with pytest.raises(_lib.Syn3rError):
        depth_correlation_loss_step(d, p)
