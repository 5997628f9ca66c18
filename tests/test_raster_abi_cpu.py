"""The scene check the four projection and the four backward entries of the rasteriser share (raster_check_scene): every family
answers a bad scene with SYN3R_E_INVALID and the same words, a short geometry buffer with SYN3R_E_WORKSPACE, before anything is
launched - no GPU is needed, the pointers are host addresses that are never followed.  (tests/test_filter3d_cpu.py holds the `_f3d`
entries to the `_ex` ones on raw / flags; this file holds all eight to one set of scene conditions.)"""
import ctypes
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

E_INVALID, E_WORKSPACE = -1, -2
DIM_MAX = 1 << 24
N, M, H, W = 16, 16, 32, 32
TAILS = {"": (), "_raw": (), "_ex": (0, 0), "_f3d": (0, 0, None)}          # what follows the common parameters, before the stream

# (changed arguments, the word the error text must hold)
BAD_SCENES = [(dict(N=0), "size"), (dict(N=-3), "size"), (dict(N=DIM_MAX + 1), "size"), (dict(means=None), "null"),
              (dict(degree=4), "sh_degree"), (dict(degree=3, coeffs=15), "coefficients"), (dict(tanfovx=0.0), "field of view")]


@pytest.fixture(scope="module")
def lib():
    from syn3r_amd import _lib, build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def calls(lib):
    """(name, call(**changes) -> rc) per entry; `P` is the forward's num_rendered_host, which no refused call may write"""
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 255) & ~255
    P = ctypes.c_longlong(-5)
    geom_need, image_need = lib.syn3r_raster_geom_bytes(N), lib.syn3r_raster_image_bytes(H, W)
    ws_need = lib.syn3r_raster_backward_workspace_bytes(N)

    def scene(means, tanfovx):
        return (means, p, p, p, p, None, 1.0, p, p, p, tanfovx, 0.5, H, W)

    def pre(entry, tail, N=N, degree=3, coeffs=M, means=p, tanfovx=0.5, geom_bytes=geom_need):
        return entry(N, degree, coeffs, *scene(means, tanfovx), p, p, geom_bytes, ctypes.byref(P), *tail, None)

    def bwd(entry, tail, N=N, degree=3, coeffs=M, means=p, tanfovx=0.5, geom_bytes=geom_need):
        return entry(N, degree, coeffs, 0, *scene(means, tanfovx), p, p, p, geom_bytes, None, p, image_need, p, None, None,
                     p, p, p, p, p, p, None, p, ws_need, *tail, None)

    out = []
    for suffix, tail in TAILS.items():
        for stage, call in (("preprocess", pre), ("backward", bwd)):
            name = f"syn3r_raster_{stage}{suffix}"
            out.append((name, lambda call=call, entry=getattr(lib, name), tail=tail, **kw: call(entry, tail, **kw)))
    assert len(out) == 8
    return out, P, buf


def test_every_entry_refuses_a_bad_scene(lib, calls):
    entries, P, _ = calls
    for name, call in entries:
        who = "raster_preprocess" if "preprocess" in name else "raster_backward"
        for changes, word in BAD_SCENES:
            rc = call(**changes)
            msg = lib.syn3r_last_error().decode()
            assert rc == E_INVALID, (name, changes, rc, msg)
            assert word in msg and msg.startswith(who + ":"), (name, changes, msg)
    assert P.value == -5


def test_every_entry_refuses_a_short_geometry_buffer(lib, calls):
    entries, P, _ = calls
    for name, call in entries:
        assert call(geom_bytes=lib.syn3r_raster_geom_bytes(N) - 1) == E_WORKSPACE, name
    assert P.value == -5
