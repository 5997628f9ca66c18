"""Mip-Splatting's 3D smoothing filter without a GPU: the closed forms of the float64 reference (tests/raster_f3d_ref.py), the
launcher flag and the trainer's defaults, the checkpoint round trip, the host-side argument checks of the three new C-ABI entries
(which reject a call before any HIP work) and the binding's mirror of the header."""
import ctypes
import io
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_aa_ref as A  # noqa: E402
import raster_f3d_ref as F  # noqa: E402
from oracle import raster_oracle as RO  # noqa: E402

E_INVALID, E_WORKSPACE = -1, -2
DIM_MAX = 1 << 24


@pytest.fixture(scope="module")
def lib():
    from syn3r_amd import _lib, build
    build.build()
    return _lib.load()


def _err(lib):
    return lib.syn3r_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- the reference
def test_reference_closed_forms():
    """One isotropic Gaussian: coef = (s^2 / (s^2 + f^2))^1.5 and s' = sqrt(s^2 + f^2); one camera: filter = sqrt(0.2) z / fx."""
    for s, f in ((0.02, 0.01), (1e-3, 0.016), (1e-6, 0.01), (0.5, 0.0)):
        sf, o = F.filtered(torch.full((1, 3), s, dtype=torch.float64), torch.tensor([0.7], dtype=torch.float64),
                           torch.tensor([f], dtype=torch.float64))
        assert float(sf[0, 0]) == pytest.approx(math.sqrt(s * s + f * f), rel=1e-14)
        assert float(o[0]) == pytest.approx(0.7 * (s * s / (s * s + f * f)) ** 1.5, rel=1e-12)
        assert math.isfinite(float(o[0])) and float(o[0]) > 0.0
    H, W = 48, 64
    view, _, _, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float64, eye=(0.1, -0.2, -1.0))
    row = F.camera_row(view, tfx, tfy, H, W)
    fx = W / (2.0 * tfx)
    assert float(row[12]) == pytest.approx(fx) and float(row[14]) == W and float(row[15]) == H
    p = torch.tensor([[0.3, -0.1, 2.5]], dtype=torch.float64)
    r = F.filter_reference(p, row[None])
    assert bool(r["seen"][0]) and float(r["filter"][0]) == pytest.approx(math.sqrt(0.2) * 3.5 / fx, rel=1e-14)
    # the nearest of several cameras decides (the largest sampling rate), whatever the order
    far = F.camera_row(RO.look_at_camera(H, W, dtype=torch.float64, eye=(0.0, 0.0, -4.0))[0], tfx, tfy, H, W)
    for tab in (torch.stack([row, far]), torch.stack([far, row])):
        assert float(F.filter_reference(p, tab)["filter"][0]) == pytest.approx(math.sqrt(0.2) * 3.5 / fx, rel=1e-14)


def test_reference_unseen_rules():
    """Behind the camera and outside the 15 % margin: unseen, filled with the largest seen filter; nothing seen: zeros, finite."""
    H, W = 40, 72
    view, _, _, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float64)
    tab = F.camera_row(view, tfx, tfy, H, W)[None]
    fx = W / (2.0 * tfx)
    x_edge = lambda z, frac: (frac * W - 0.5 * W) * z / fx          # the x whose pixel is frac * W
    p = torch.tensor([[0.0, 0.0, 2.0], [0.0, 0.0, 5.0], [0.0, 0.0, -1.0], [0.0, 0.0, 0.1], [x_edge(3.0, 1.2), 0.0, 3.0],
                      [x_edge(3.0, 1.1), 0.0, 3.0], [x_edge(3.0, -0.2), 0.0, 3.0]], dtype=torch.float64)
    r = F.filter_reference(p, tab)
    assert r["seen"].tolist() == [True, True, False, False, False, True, False]
    big = math.sqrt(0.2) * 5.0 / fx
    assert float(r["filter"][1]) == pytest.approx(big, rel=1e-14)
    for k in (2, 3, 4, 6):
        assert float(r["filter"][k]) == pytest.approx(big, rel=1e-14)
    none = F.filter_reference(p[[2, 3, 4]], tab)
    assert not bool(none["seen"].any()) and none["filter"].tolist() == [0.0, 0.0, 0.0]


def test_reference_scenes_stay_under_the_radius_edge_cap():
    """At most 1 % of a scene's Gaussians may sit within 1e-4 of an integer radius argument and be taken out; the filters of the
    scenes are finite, positive and of the order of the scales (the filter matters at every shape)."""
    for shape in A.SHAPES:
        sc = F.scene(shape)
        assert sc["dropped"] <= 0.01 * sc["N0"], (shape, sc["dropped"])
        assert sc["N"] == sc["N0"] - sc["dropped"] and sc["f"].shape == (sc["N"],)
        assert bool(torch.isfinite(sc["f"]).all()) and float(sc["f"].min()) > 0.0
        assert 0.1 * shape[5] < float(sc["f"].median()) < 10.0 * shape[5]


def test_property_scene_premise():
    """The premise of the GPU test of the property, on the reference alone: with the filter the close-up's alpha has a per-axis second
    moment of at least (filter fx / 0.25)^2, without it far less; and under an opacity <= 1 the filtered Gaussian is not drawn."""
    sc, f, fx, coef = F.property_scene()
    bound = (float(f[0]) * fx / F.PROP["z_close"]) ** 2
    assert coef == pytest.approx(2.366e-4, rel=1e-3) and bound == pytest.approx(12.8, rel=1e-9)
    with torch.no_grad():
        (_, _, _, a_on, _), _ = F.rasterize(sc, 0, f, False)
        (_, _, _, a_off, _), _ = F.rasterize(sc, 0, torch.zeros_like(f), False)
        phys = dict(sc, o=torch.tensor([0.95], dtype=torch.float64))
        (_, _, _, a_phys_on, _), _ = F.rasterize(phys, 0, f, False)
        (_, _, _, a_phys_off, _), _ = F.rasterize(phys, 0, torch.zeros_like(f), False)
    assert F.second_moment(a_on) >= bound and F.second_moment(a_on) < 1.02 * (bound + 0.3 + 0.05)
    assert F.second_moment(a_off) < 0.2 * bound
    assert float(a_phys_on.max()) == 0.0                             # coef 2.4e-4: below the 1/255 cut
    assert 0.25 < F.second_moment(a_phys_off) < 0.45                 # the dilation's 0.3 px^2 (+ 0.05 of the Gaussian itself)


# ---------------------------------------------------------------------------------------------------------------- flags, defaults
def test_launcher_flag_and_trainer_defaults():
    import dataclasses
    from syn3r_amd import launch
    from syn3r_amd.gs import OptimizationParams
    o = OptimizationParams()
    assert (o.filter_3d, o.filter_3d_variance, o.filter_3d_interval) == (False, 0.2, 100)
    a = launch.parse(["--scenes", "x", "--filter_3d", "1"])
    assert a.filter_3d == 1 and a.ignored_flags == []
    assert launch.parse(["--scenes", "x"]).filter_3d == 0
    assert "--filter_3d" not in launch.FSGS_FLAGS
    on = launch.apply_trainer_flags(OptimizationParams(), a)
    assert on.filter_3d is True and on.antialiasing is False
    assert dataclasses.replace(on, filter_3d=False) == OptimizationParams()          # nothing else moved
    assert launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x"])).filter_3d is False
    assert launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x", "--filter_3d", "0"])).filter_3d is False
    kept = launch.apply_trainer_flags(OptimizationParams(filter_3d=True), launch.parse(["--scenes", "x", "--filter_3d", "0"]))
    assert kept.filter_3d is True                                    # 0 leaves the field as `opt` has it, as --antialiasing
    both = launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x", "--filter_3d", "1", "--antialiasing", "1"]))
    assert both.filter_3d is True and both.antialiasing is True
    for bad in (["--filter_3d", "2"], ["--filter_3"], ["--filter3d", "1"]):
        with pytest.raises(SystemExit):
            launch.parse(["--scenes", "x"] + bad)


def _cpu_model(n=12, seed=0):
    from syn3r_amd.gs.trainer import GaussianModel
    g = np.random.default_rng(seed)
    return GaussianModel(g.normal(size=(n, 3)).astype(np.float32), np.log(g.uniform(0.002, 0.05, size=(n, 3))).astype(np.float32),
                         g.normal(size=(n, 4)).astype(np.float32), g.normal(size=n).astype(np.float32),
                         g.normal(size=(n, 16, 3)).astype(np.float32), device="cpu")


def test_checkpoint_round_trip_with_and_without_a_filter():
    gm = _cpu_model()
    assert gm.filter_3D is None
    plain = gm.capture()
    assert sorted(plain) == ["active_sh_degree", "confidence", "features", "opacity", "rotation", "scaling", "xyz"]
    # byte-compatible: what torch.save writes for a model without a filter does not depend on the new attribute
    a, b = io.BytesIO(), io.BytesIO()
    torch.save((plain, 7), a)
    torch.save((dict(active_sh_degree=gm.active_sh_degree, xyz=gm._xyz.detach().clone(), features=gm._features.detach().clone(),
                     scaling=gm._scaling.detach().clone(), rotation=gm._rotation.detach().clone(),
                     opacity=gm._opacity.detach().clone(), confidence=gm.confidence.clone()), 7), b)
    assert a.getvalue() == b.getvalue()
    gm.filter_3D = torch.linspace(0.01, 0.02, 12)
    state = gm.capture()
    assert torch.equal(state["filter_3D"], gm.filter_3D) and state["filter_3D"] is not gm.filter_3D
    buf = io.BytesIO()
    torch.save((state, 3), buf)
    buf.seek(0)
    loaded, it = torch.load(buf, weights_only=True)
    other = _cpu_model(seed=1)
    other.restore(loaded)
    assert it == 3 and torch.equal(other.filter_3D, gm.filter_3D) and torch.equal(other._xyz, gm._xyz)
    other.restore(plain)                                             # an old checkpoint: the filter goes
    assert other.filter_3D is None
    other.filter_3D = torch.ones(12)
    other.set_from_pcd(np.random.default_rng(2).normal(size=(3, 3)), np.full((3, 3), 0.5), append=False)
    assert other.filter_3D is None


def test_option_off_touches_nothing_and_on_has_no_cpu_fallback():
    from syn3r_amd import _lib
    from syn3r_amd.gs.trainer import GSTrainer, OptimizationParams
    from syn3r_amd.gs.train_ops import compute_filter_3D
    tr = GSTrainer(_cpu_model(), [], OptimizationParams())
    assert tr.ensure_filter_3D() is None and tr.gaussians.filter_3D is None and tr.filter_3d_computes == 0
    with pytest.raises(_lib.Syn3rError):
        compute_filter_3D(torch.rand(8, 3), torch.rand(2, 16))
    # a trainer without cameras: all-zero filters (nothing is seen), no launch
    tr = GSTrainer(_cpu_model(), [], OptimizationParams(filter_3d=True))
    f = tr.ensure_filter_3D()
    assert f is tr.gaussians.filter_3D and f.tolist() == [0.0] * 12 and tr.filter_3d_computes == 1
    assert tr.ensure_filter_3D() is f and tr.filter_3d_computes == 1
    # density control changes the set: the filter is dropped with it (a prune after a clone may give the old N back)
    tr.density._keep_gaussians(torch.ones(12, dtype=torch.bool))
    assert tr.gaussians.filter_3D is None


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_filter_entry_rejects_bad_arguments(lib):
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 255) & ~255      # never dereferenced: every call below is rejected
    n, c = 64, 3
    need = lib.syn3r_filter3d_workspace_bytes(n)
    assert need > 0 and need % 256 == 0
    for bad in (0, -1, DIM_MAX + 1):
        assert lib.syn3r_filter3d_workspace_bytes(bad) == 0

    def call(xyz=p, n_=n, cams=p, c_=c, var=0.2, near=0.2, margin=0.15, out=p, ws=p, wsb=need):
        return lib.syn3r_filter3d_compute(xyz, n_, cams, c_, var, near, margin, out, ws, wsb, None)

    for kw in (dict(xyz=None), dict(cams=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == E_INVALID and "null" in _err(lib), kw
    for bad in (0, -7, DIM_MAX + 1):
        assert call(n_=bad) == E_INVALID and f"n={bad}" in _err(lib)
        assert call(c_=bad) == E_INVALID and f"n_cams={bad}" in _err(lib)
    for kw, word in ((dict(var=0.0), "variance"), (dict(var=-1.0), "variance"), (dict(var=float("nan")), "variance"),
                     (dict(var=float("inf")), "variance"), (dict(near=0.0), "near"), (dict(near=float("nan")), "near"),
                     (dict(margin=-0.1), "margin"), (dict(margin=float("nan")), "margin")):
        assert call(**kw) == E_INVALID and word in _err(lib), kw
    assert call(wsb=need - 1) == E_WORKSPACE and "workspace" in _err(lib)
    assert call(wsb=0) == E_WORKSPACE
    assert call(ws=p + 2) == E_INVALID and "aligned" in _err(lib)


def test_raster_f3d_entries_validate_as_the_ex_entries(lib):
    """raw, flags, sizes, null pointers and short buffers: the `_f3d` entries answer as the `_ex` entries do, with or without a
    filter pointer, before anything is launched."""
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 255) & ~255
    N, M, H, W = 16, 16, 32, 32
    P = ctypes.c_longlong(-5)
    geom_need = lib.syn3r_raster_geom_bytes(N)

    def pre(entry, tail, N_=N, means=p, flt=(), geom_bytes=geom_need):
        return entry(N_, 3, M, means, p, p, p, p, None, 1.0, p, p, p, 0.5, 0.5, H, W, p, p, geom_bytes, ctypes.byref(P), *tail, *flt, None)

    def bwd(entry, tail, N_=N, means=p, flt=(), ws_bytes=None):
        ws_bytes = lib.syn3r_raster_backward_workspace_bytes(N) if ws_bytes is None else ws_bytes
        return entry(N_, 3, M, 0, means, p, p, p, p, None, 1.0, p, p, p, 0.5, 0.5, H, W, p, p, p, geom_need, None, p,
                     lib.syn3r_raster_image_bytes(H, W), p, None, None, p, p, p, p, p, p, None, p, ws_bytes, *tail, *flt, None)

    for flt in (None, p):
        for call, ex, f3 in ((pre, lib.syn3r_raster_preprocess_ex, lib.syn3r_raster_preprocess_f3d),
                             (bwd, lib.syn3r_raster_backward_ex, lib.syn3r_raster_backward_f3d)):
            for kw, tail, word in ((dict(), (0, 2), "flag"), (dict(), (1, 1 << 30), "flag"), (dict(), (0, -2), "flag"), (dict(), (2, 0), "raw"),
                                   (dict(), (-1, 1), "raw"), (dict(N_=0), (0, 0), "size"), (dict(N_=-3), (1, 1), "size"),
                                   (dict(means=None), (0, 1), "null")):
                rc_ex = call(ex, tail, **kw)
                msg_ex = _err(lib)
                rc_f3 = call(f3, tail, flt=(flt,), **kw)
                msg_f3 = _err(lib)
                assert rc_ex == rc_f3 == E_INVALID, (kw, tail)
                assert word in msg_ex and word in msg_f3, (kw, tail, msg_ex, msg_f3)
        assert pre(lib.syn3r_raster_preprocess_f3d, (0, 1), flt=(flt,), geom_bytes=geom_need - 1) == E_WORKSPACE
        assert bwd(lib.syn3r_raster_backward_f3d, (1, 0), flt=(flt,), ws_bytes=1) == E_WORKSPACE
    assert P.value == -5


def _params(decl):
    inside = decl[decl.index("(") + 1:decl.rindex(")")]
    return [a.strip() for a in inside.split(",")]


def test_binding_mirrors_the_header():
    from syn3r_amd import _lib
    text = (ROOT / "include" / "syn3r_hip.h").read_text()
    decls = {m.group(1): m.group(0) for m in re.finditer(r"(?:int|size_t)\s+(syn3r_\w+)\s*\([^;{]*\)\s*;", text)}
    kinds = {_lib.c_i: "int", _lib.c_f: "float", _lib.c_sz: "size_t", _lib.c_ll: "long long"}
    for name in ("syn3r_filter3d_workspace_bytes", "syn3r_filter3d_compute", "syn3r_raster_preprocess_f3d", "syn3r_raster_backward_f3d"):
        assert name in decls and name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        params = _params(decls[name])
        assert len(params) == len(args), (name, len(params), len(args))
        for par, typ in zip(params, args):
            if "*" in par:
                assert typ is _lib.c_p or typ is ctypes.POINTER(_lib.c_ll), (name, par)
            else:
                assert par.rsplit(" ", 1)[0].strip() == kinds[typ], (name, par)
    # the `_f3d` entries are the `_ex` entries plus ONE pointer before the stream
    for a, b in (("syn3r_raster_preprocess_ex", "syn3r_raster_preprocess_f3d"), ("syn3r_raster_backward_ex", "syn3r_raster_backward_f3d")):
        pa, pb = _params(decls[a]), _params(decls[b])
        assert pb[:-2] == pa[:-1] and pb[-2] == "const float* filter3d" and pb[-1] == pa[-1] == "void* stream"
        assert _lib.SIGNATURES[b][1] == _lib.SIGNATURES[a][1][:-1] + [_lib.c_p, _lib.c_p]
    assert (_lib.FILTER3D_VARIANCE, _lib.FILTER3D_NEAR, _lib.FILTER3D_MARGIN) == (F.VARIANCE, F.NEAR, F.MARGIN) == (0.2, 0.2, 0.15)
    for const in ("variance = 0.2", "near = 0.2", "margin = 0.15", "UNPINNED"):
        assert const in text[text.index("syn3r_filter3d_compute - "):text.index("size_t syn3r_filter3d_workspace_bytes")], const
