"""Uninitialised memory: every op of the public Python surface under poisoned allocations (tests/poison.py), and the rasteriser on
scenes of one, two and three Gaussians.

The wrappers of syn3r_amd allocate outputs and state with `torch.empty*` and scratch through `_lib.workspace()`.  A test process is
short, so those buffers are in practice zero and a kernel that reads a word before anything wrote it - or skips an output row, or
trusts a flag nobody cleared - passes every other test of the suite.  Here each op runs three times, with every such buffer full of
0x00, of 0xFF (NaN, -1) and of 0x3C (fp32 0.0115, fp16 1.0586, int32 1010580540), and has to

  * be finite where its reference is,
  * pass the reference check of its OWN test module under every pattern (the rows import that module's helpers, references and, where
    the module keeps inputs, run and bars in one function, call that test function itself inside the poisoned block - no tolerance is
    restated here except the rasteriser's three image bars, which tests/test_raster_gpu.py holds as literals), and
  * give the same bits under the three patterns, unless it accumulates with float atomics.

Bit-compared: rasteriser forward (images, radii, tile lists, n_contrib), sort_pairs, the neighbour search, the outlier filter, the 3D
filter, every loss and its step form, image_metrics, the scheduler's step_interp_prob_uncertain and step_interp without the gradient,
the inverse warps, warp_post / fuse_uncertainty, flow_cycle_mask, every UNet op, LPIPS value and gradient.
Tolerance-only (float atomics: the order of the additions changes from run to run, csrc/raster_bwd.hip, csrc/warp.hip, csrc/sched.hip
`unsafeAtomicAdd`): the rasteriser backward, forward_warp, step_interp with the gradient (its standard deviation sums).  They get the
reference check, the finite check and, the backward, "rows of culled Gaussians are exactly zero".

No test here aims at a fault: every consumer of a poisoned word was read in the kernel sources first (the findings are in the commit
message), and the shapes are the smallest of each module."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_aa_ref as A  # noqa: E402
import raster_absgrad_ref as AB  # noqa: E402
import raster_f3d_ref as F  # noqa: E402
from oracle import raster_oracle as RO  # noqa: E402
from poison import PATTERNS, Row, poisoned, run_row  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"

# tests/test_raster_gpu.py::test_forward_vs_oracle / test_backward_vs_autograd (literals there; the same in test_raster_aa_gpu.py,
# test_filter3d_gpu.py and, as BAR, test_raster_absgrad_gpu.py)
COLOR_ATOL = ALPHA_ATOL = 2e-4
DEPTH_ATOL, DEPTH_RTOL = 1e-3, 1e-4
GRAD_BAR = 2e-3
MODES = ("plain", "aa", "f3d", "raw")


def _no_measurements(*a, **k):
    """stands in for the `measurements` fixture where an existing test function is called as a row's reference check"""


# ======================================================================================================== rasteriser
def _filter_of(sc):
    return F.filter_reference(sc["m"], F.scene_cameras(sc["H"], sc["W"]))["filter"]


def _forward(sc, dev, deg, mode, debug=False):
    """rasterize_forward in one of MODES: -> (color, radii, depth, alpha, state)"""
    import test_raster_aa_gpu as TA
    from syn3r_amd.raster import rasterize_forward
    f = lambda t: t.to(dev, torch.float32).contiguous()
    raw = mode == "raw"
    p = F.raw_params(sc) if raw else sc
    cf = f(sc["cf"]) if sc["cf"] is not None else None
    with torch.no_grad():
        return rasterize_forward(f(sc["m"]), f(sc["sh"]), f(p["o"]), f(p["s"]), f(p["q"]), cf, TA.settings(sc, dev, deg, mode == "aa", debug),
                                 raw_params=raw, filter_3D=f(sc["f"]) if mode == "f3d" else None)


def _backward(st, dev, weights, with_abs, with_dz):
    """rasterize_backward -> (dict of gradients by A.PARAMS name (+ "cf"), d_means2D, abs [N,2] or None)"""
    from syn3r_amd.raster import rasterize_backward
    wc, wd, wa = (w.to(dev, torch.float32).contiguous() for w in weights)
    N = st.scene[0]
    buf = torch.empty((N, 2), dtype=torch.float32, device=dev) if with_abs else None      # (poisoned: every row has to be written)
    with torch.no_grad():
        d_m3, d_m2, d_sh, d_op, d_sc, d_ro, d_cf = rasterize_backward(st, wc, wd if with_dz else None, wa if with_dz else None,
                                                                      abs_grad_out=buf)
    got = dict(m=d_m3, s=d_sc, q=d_ro, o=d_op.reshape(-1), sh=d_sh)
    if d_cf is not None:
        got["cf"] = d_cf
    return got, d_m2, buf


def _weights(H, W, with_dz):
    wc, wd, wa = A.loss_weights(H, W)
    return (wc, wd, wa) if with_dz else (wc, torch.zeros_like(wd), torch.zeros_like(wa))


_ref_cache = {}


def _reference(key, sc, deg, mode, with_dz=True, grads=True):
    """float64 render of `sc` in `mode` (the plain oracle, raster_aa_ref or raster_f3d_ref; "raw" is the plain render and, for the
    gradients, the activations' chain rule of raster_f3d_ref.reference), the gradients of sum(wc colour) + sum(wd depth) + sum(wa alpha)
    and AbsGS' absolute gradient (raster_absgrad_ref).  Computed once per key; nobody modifies it."""
    key = (key, mode, with_dz, grads)
    if key in _ref_cache:
        return _ref_cache[key]
    weights = _weights(sc["H"], sc["W"], with_dz)
    if mode == "f3d":
        (oc, orad, od, oa, aux), p = F.rasterize(sc, deg, sc["f"], False, requires_grad=grads)
    else:
        (oc, orad, od, oa, aux), p, _, _ = A.rasterize(sc, deg, mode == "aa", requires_grad=grads, conf_grad=True)
    ref = dict(color=oc.detach(), depth=od.detach(), alpha=oa.detach(), radii=orad, aux=aux, valid=aux["pre"]["valid"], weights=weights)
    if grads:
        wc, wd, wa = weights
        ((oc * wc).sum() + (od * wd).sum() + (oa * wa).sum()).backward()
        g = {k: p[k].grad.clone() for k in A.PARAMS}
        if sc["cf"] is not None:
            g["cf"] = p["cf"].grad.clone()
        if mode == "raw":
            raw = F.raw_params(sc)
            qn = sc["q"] / sc["q"].norm(dim=1, keepdim=True)
            gq = g["q"]
            g["s"] = g["s"] * sc["s"]
            g["o"] = g["o"] * sc["o"] * (1.0 - sc["o"])
            g["q"] = (gq - qn * (qn * gq).sum(1, keepdim=True)) / raw["q"].norm(dim=1, keepdim=True)
        ref["grads"] = g
        ref["abs"] = AB.from_aux(sc, aux, weights)["abs"]
    _ref_cache[key] = ref
    return ref


def _image_errors(outs, ref):
    color, depth, alpha = outs
    return {k: float((a.cpu().double() - b).abs().max()) for k, a, b in (("color", color, ref["color"]), ("depth", depth, ref["depth"]),
                                                                       ("alpha", alpha, ref["alpha"]))}


def _check_images(color, depth, alpha, ref):
    np.testing.assert_allclose(color.cpu().numpy(), ref["color"].numpy(), atol=COLOR_ATOL)
    np.testing.assert_allclose(alpha.cpu().numpy(), ref["alpha"].numpy(), atol=ALPHA_ATOL)
    np.testing.assert_allclose(depth.cpu().numpy(), ref["depth"].numpy(), atol=DEPTH_ATOL, rtol=DEPTH_RTOL)


def _grad_errors(got, want):
    err = {}
    for k, b in want.items():
        a = got[k]
        assert torch.isfinite(a).all(), k
        err[k] = (a.cpu().double() - b.reshape(a.shape)).abs().max().item() / (b.abs().max().item() + 1e-12)
    return err


def _check_backward(got, d_m2, buf, radii, ref, tag):
    """the bars of tests/test_raster_gpu.py::test_backward_vs_autograd and test_raster_absgrad_gpu.py::compare, and exact zeros on
    the rows of culled Gaussians"""
    assert set(got) == set(ref["grads"]), (tag, sorted(got))
    err = _grad_errors(got, ref["grads"])
    for k, v in err.items():
        assert v < GRAD_BAR, (tag, k, v)
    culled = radii == 0
    for k, a in list(got.items()) + [("means2D", d_m2)] + ([("abs", buf)] if buf is not None else []):
        assert torch.isfinite(a).all(), (tag, k)
        if bool(culled.any()):
            assert float(a[culled].abs().max()) == 0.0, (tag, k)
    assert (d_m2[:, 2] == 0).all(), tag
    if buf is not None:
        assert bool((buf >= 0).all()), tag
        for c in (0, 1):
            e = float((buf[:, c].cpu().double() - ref["abs"][:, c]).abs().max()) / (float(ref["abs"][:, c].abs().max()) + 1e-12)
            err[f"abs{c}"] = e
            assert e < GRAD_BAR, (tag, "abs", c, e)
    return err


# ---------------------------------------------------------------------------------------------- forward rows of the sweep
def _debug_outputs(out):
    from syn3r_amd.raster import _Rasterize
    color, radii, depth, alpha = out[:4]
    dbg = _Rasterize.debug_state
    return (color, depth, alpha, radii, dbg["point_list"], dbg["ranges"], dbg["n_contrib"])


_oracle_cache = {}


def _oracles(tag, sc, deg):
    """the float64 oracle render (images, n_contrib) and the float32 one (tile lists, as tests/test_raster_gpu.py::
    test_tile_lists_bit_exact compares them), once per scene"""
    import test_raster_gpu as TR
    if tag not in _oracle_cache:
        with torch.no_grad():
            (oc, orad, od, oa, aux64), _ = TR.oracle_render(sc, torch.float64, deg=deg)
            (_, _, _, _, aux32), _ = TR.oracle_render(sc, torch.float32, deg=deg)
        _oracle_cache[tag] = dict(color=oc, depth=od, alpha=oa, radii=orad, aux64=aux64, aux32=aux32)
    return _oracle_cache[tag]


def _check_forward(outs, ora, culled_first=10):
    """tests/test_raster_gpu.py::test_forward_vs_oracle and ::test_tile_lists_bit_exact on one debug render"""
    color, depth, alpha, radii, plist, ranges, n_contrib = outs
    rd = (radii.cpu().long() - ora["radii"]).abs()
    assert (rd > 0).float().mean() < 5e-3 and rd.max() <= 1
    assert (radii[:culled_first] == 0).all()
    _check_images(color, depth, alpha, ora)
    assert float(alpha.max()) > 0.5
    np.testing.assert_array_equal(plist.cpu().numpy(), ora["aux32"]["point_list"])
    np.testing.assert_array_equal(ranges.cpu().numpy(), ora["aux32"]["ranges"])
    assert (n_contrib.cpu().numpy() != ora["aux64"]["n_contrib"]).mean() < 1e-3


def _forward_row(N, H, W, conf):
    import test_raster_gpu as TR
    sc = TR.scene(N, H, W, seed=N + H, conf=conf)
    tag = ("fwd", N, H, W, conf)

    def run(dev):
        with torch.no_grad():
            out, _, _ = TR.hip_render(sc, dev, deg=3)          # (debug=True: sync pair count, the binning state is exposed)
        return _debug_outputs(out)

    return Row(f"raster_forward N{N} {H}x{W}", run, True, lambda outs: _check_forward(outs, _oracles(tag, sc, 3)))


# The pair sort takes an image of more than kMaxSuper = 512 super-tiles of 8 x 8 tiles (csrc/raster_bin.hip bin_plan: ss <= 3), a side
# is at most 2^15 pixels (SYN3R_SIDE_MAX): ceil(gx / 8) * ceil(gy / 8) >= 513 with the fewest pixels is 171 x 3 super-tiles, 1361 x 17
# tiles, 21761 x 257 pixels (5.6 M; 170 x 3 = 510 still takes the hierarchical binning).  The ceiling is the 8192 x 1152 case of
# tests/test_raster_full_gpu.py (9.4 M pixels).
PAIR_SORT_H, PAIR_SORT_W = 2 * 128 + 1, 170 * 128 + 1


def _pair_sort_row():
    import test_raster_full_gpu as TRF
    N, H, W, bg = 500, PAIR_SORT_H, PAIR_SORT_W, (0.1, 0.2, 0.3)
    m, s, q, o, sh = RO.synthetic_gaussians(N, seed=1234, dtype=torch.float32)       # (_check_tile_lists' scene)

    def run(dev):
        with torch.no_grad():
            out, _, _ = TRF._render(dev, m, s, q, o, sh, H, W, bg, False, True)
        outs = _debug_outputs(out)
        assert int((outs[3] > 0).sum()) > 10 and outs[4].numel() > 1000        # something is drawn
        return outs

    return Row("raster_forward pair-sort fallback", run, True, lambda outs: TRF._check_tile_lists(outs[0].device, N, H, W, bg))


def _async_row():
    """the second call of a shape in async mode runs on the device-side pair count, with the capacity of the first"""
    import test_raster_gpu as TR
    from syn3r_amd import raster
    N, H, W = 300, 40, 72
    sc = TR.scene(N, H, W, seed=N + H, conf=True)
    tag = ("fwd", N, H, W, True)

    def run(dev):
        from syn3r_amd.raster import GaussianRasterizationSettings, GaussianRasterizer
        f = lambda t: t.to(dev, torch.float32)
        st = GaussianRasterizationSettings(H, W, sc["tfx"], sc["tfy"], f(sc["bg"]), 1.0, f(sc["view"]), f(sc["proj"]), 3, f(sc["campos"]),
                                           False, False)
        call = lambda: GaussianRasterizer(st)(f(sc["m"]), None, f(sc["o"]), shs=f(sc["sh"]), scales=f(sc["s"]), rotations=f(sc["q"]),
                                              confidence=f(sc["cf"]))
        key = raster.capacity_key(dev, N, H, W)
        raster.set_pair_count_mode("async")
        try:
            raster._capacity.pop(key, None)
            with torch.no_grad():
                call()
                assert key in raster._capacity and key not in raster._pending
                color, radii, depth, alpha = call()
                assert len(raster._pending[key]) == 1                      # this one was not read back
            raster.flush_pair_checks()                                     # ... and did not overflow
        finally:
            raster._pending.clear()
            raster.set_pair_count_mode("sync")
        return color, depth, alpha, radii

    def check(outs):
        color, depth, alpha, radii = outs
        ora = _oracles(tag, sc, 3)
        _check_images(color, depth, alpha, ora)
        assert (radii[:10] == 0).all() and float(alpha.max()) > 0.5

    return Row("raster_forward async second call", run, True, check)


FORWARD_ROWS = [lambda: _forward_row(300, 40, 72, True), lambda: _forward_row(2000, 100, 260, False), _pair_sort_row, _async_row]


@pytest.mark.parametrize("make", FORWARD_ROWS, ids=["N300_40x72_conf", "N2000_100x260_ragged", "pair_sort_fallback", "async_second_call"])
def test_raster_forward_rows(make, gpu, monkeypatch):
    run_row(make(), monkeypatch, gpu)


def test_pair_sort_row_is_the_smallest_fallback_image():
    """the bound of csrc/raster_bin.hip restated: 512 super-tiles of at most 8 x 8 tiles of 16 x 16 pixels"""
    supers = lambda H, W: math.ceil(math.ceil(W / 16) / 8) * math.ceil(math.ceil(H / 16) / 8)
    assert supers(PAIR_SORT_H, PAIR_SORT_W) == 513 and supers(PAIR_SORT_H - 1, PAIR_SORT_W) <= 512 and supers(PAIR_SORT_H, PAIR_SORT_W - 1) <= 512
    assert PAIR_SORT_H * PAIR_SORT_W < 1152 * 8192 and max(PAIR_SORT_H, PAIR_SORT_W) <= 1 << 15
    best = min((128 * (a - 1) + 1) * (128 * (b - 1) + 1) for a in range(1, 257) for b in range(1, 257) if a * b > 512)
    assert PAIR_SORT_H * PAIR_SORT_W == best


# ---------------------------------------------------------------------------------------------- backward rows of the sweep
def _backward_scene():
    import test_raster_gpu as TR
    sc = TR.scene(300, 40, 72, seed=7 * 300, conf=True)          # test_backward_vs_autograd's smallest case
    sc["f"] = _filter_of(sc)
    return sc


@pytest.mark.parametrize("mode", MODES)
def test_raster_backward_rows(mode, gpu, monkeypatch, measurements):
    """300 Gaussians on 40 x 72 (ten of them culled), every gradient and AbsGS' buffer: with and without `abs_grad_out`, with and
    without depth / alpha gradients.  Float atomics: tolerance-only."""
    sc, deg = _backward_scene(), 3
    variants = [(a, z) for a in (False, True) for z in (False, True)]

    def run(dev):
        outs = []
        for with_abs, with_dz in variants:
            _, radii, _, _, st = _forward(sc, dev, deg, mode)
            got, d_m2, buf = _backward(st, dev, _weights(sc["H"], sc["W"], with_dz), with_abs, with_dz)
            outs.append((got, d_m2, buf, radii))
        run.last = outs
        return tuple(t for got, d_m2, buf, _ in outs for t in list(got.values()) + [d_m2] + ([buf] if buf is not None else []))

    def check(_outs):
        for (with_abs, with_dz), (got, d_m2, buf, radii) in zip(variants, run.last):
            assert int((radii == 0).sum()) >= 10
            ref = _reference("bwd300", sc, deg, mode, with_dz)
            err = _check_backward(got, d_m2, buf, radii, ref, (mode, with_abs, with_dz))
            measurements("uninit_raster_backward", mode=mode, with_abs=with_abs, with_dz=with_dz, **err)

    run_row(Row(f"raster_backward {mode}", run, False, check), monkeypatch, gpu)


# ---------------------------------------------------------------------------------------------- one, two and three Gaussians
TINY_SIZES = [(16, 16), (5, 7), (33, 50)]           # one tile, a partial tile, 3 x 4 tiles with partial ones on both edges
RADIUS_EDGE = 1e-3


def tiny_scene(N, H, W):
    m, s, q, o, sh = RO.synthetic_gaussians(N, seed=N, dtype=torch.float64, log_scale_mean=math.log(0.3))
    view, proj, campos, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float64)
    bg = torch.tensor([0.1, 0.3, 0.7], dtype=torch.float64)
    sc = dict(m=m, s=s, q=q, o=o, sh=sh, cf=None, view=view, proj=proj, campos=campos, tfx=tfx, tfy=tfy, bg=bg, H=H, W=W, N=N)
    sc["f"] = _filter_of(sc)
    return sc


def _tiny_reference(sc, mode):
    ref = _reference(("tiny", sc["N"], sc["H"], sc["W"]), sc, 3, mode)
    # nothing is culled, and no 3 sqrt(lambda) sits where an fp32 ceil() could land on the other integer
    arg = 3.0 * torch.sqrt(F.lam_max(ref["aux"]["pre"]["conic"].detach()))
    assert bool(ref["valid"].all()) and int(ref["radii"].min()) >= 3
    assert float((arg - torch.round(arg)).abs().min()) >= RADIUS_EDGE
    assert 1 <= len(ref["aux"]["point_list"]) <= 40 and (0.4 if mode in ("plain", "raw") else 0.05) < float(ref["alpha"].max()) < 0.8
    return ref


def _async_renders(sc, dev, mode, calls=3):
    """`calls` renders of the shape in async mode (the first sizes exactly, the others run on the device-side count), then
    flush_pair_checks(), which must not raise"""
    from syn3r_amd import raster
    key = raster.capacity_key(dev, sc["N"], sc["H"], sc["W"])
    raster.set_pair_count_mode("async")
    try:
        raster._capacity.pop(key, None)
        outs = [_forward(sc, dev, 3, mode)[:4] for _ in range(calls)]
        assert len(raster._pending.get(key, [])) <= calls - 1       # (a later call may already have examined an earlier one)
        assert raster.flush_pair_checks() == 0
    finally:
        raster._pending.clear()
        raster.set_pair_count_mode("sync")
    return outs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W", TINY_SIZES, ids=[f"{h}x{w}" for h, w in TINY_SIZES])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_tiny_scene(N, H, W, mode, gpu, monkeypatch, measurements):
    """N < 4 Gaussians, nothing culled: k_preprocess' first block has fewer live threads than the geometry header has words.  Forward
    (sync with the binning state exposed, and three async calls) and backward against the float64 references at the bars of
    tests/test_raster_gpu.py; radii and tile lists exactly; the forward bit for bit across the patterns."""
    sc = tiny_scene(N, H, W)
    ref = _tiny_reference(sc, mode)
    tag = f"tiny N{N} {H}x{W} {mode}"

    def run_fwd(dev):
        out = _forward(sc, dev, 3, mode, debug=True)
        outs = _debug_outputs(out)
        a_outs = _async_renders(sc, dev, mode)
        for c, r, d, a in a_outs:
            assert torch.equal(c, outs[0]) and torch.equal(d, outs[1]) and torch.equal(a, outs[2]) and torch.equal(r, outs[3]), tag
        return outs

    def check_fwd(outs):
        color, depth, alpha, radii, plist, ranges, n_contrib = outs
        err = _image_errors((color, depth, alpha), ref)
        measurements("uninit_tiny_forward", N=N, H=H, W=W, mode=mode, **err)
        assert torch.equal(radii.cpu().long(), ref["radii"].long()), (radii.tolist(), ref["radii"].tolist())
        np.testing.assert_array_equal(plist.cpu().numpy(), ref["aux"]["point_list"])
        np.testing.assert_array_equal(ranges.cpu().numpy(), ref["aux"]["ranges"])
        _check_images(color, depth, alpha, ref)

    def run_bwd(dev):
        _, radii, _, _, st = _forward(sc, dev, 3, mode)
        run_bwd.last = _backward(st, dev, ref["weights"], True, True) + (radii,)
        got, d_m2, buf, _ = run_bwd.last
        return tuple(got.values()) + (d_m2, buf)

    def check_bwd(_outs):
        got, d_m2, buf, radii = run_bwd.last
        err = _check_backward(got, d_m2, buf, radii, ref, tag)
        assert float(d_m2.abs().sum()) > 0
        measurements("uninit_tiny_backward", N=N, H=H, W=W, mode=mode, **err)

    run_row(Row(tag + " forward", run_fwd, True, check_fwd), monkeypatch, gpu)
    run_row(Row(tag + " backward", run_bwd, False, check_bwd), monkeypatch, gpu)


# ---------------------------------------------------------------------------------------------- the geometry header, C ABI
def _abi_render(sc, dev, fill):
    """syn3r_raster_preprocess_f3d + syn3r_raster_render on state buffers the TEST fills with `fill` (include/syn3r_hip.h puts no
    "must be zeroed" duty on the caller): -> (the four header words, exact pair count read back, colour)"""
    from syn3r_amd import _lib as L
    lib = L.load()
    f = lambda t: t.float().to(dev).contiguous()
    N, H, W = sc["N"], sc["H"], sc["W"]
    m3, s, q, o, sh = f(sc["m"]), f(sc["s"]), f(sc["q"]), f(sc["o"]), f(sc["sh"])
    host = lambda t: L.host_f32(t.double().reshape(-1).tolist())
    view, proj, campos, bg = host(sc["view"].float()), host(sc["proj"].float()), host(sc["campos"].float()), host(sc["bg"].float())
    stream = L.stream_ptr(dev)
    u8 = lambda n: torch.full((max(int(n), 256),), fill, dtype=torch.uint8, device=dev)
    geom, image = u8(lib.syn3r_raster_geom_bytes(N)), u8(lib.syn3r_raster_image_bytes(H, W))
    radii = torch.full((N,), -1, dtype=torch.int32, device=dev)
    P = C.c_longlong(0)
    L.check(lib.syn3r_raster_preprocess_f3d(N, 3, sh.shape[1], L.ptr(m3), L.ptr(s), L.ptr(q), L.ptr(o), L.ptr(sh), None, 1.0, view, proj, campos,
                                            float(sc["tfx"]), float(sc["tfy"]), H, W, L.ptr(radii), L.ptr(geom), geom.numel(), C.byref(P),
                                            0, 0, None, stream), "syn3r_raster_preprocess_f3d")
    P = int(P.value)
    binning = u8(lib.syn3r_raster_binning_bytes(P))
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    color, depth, alpha = new(3, H, W), new(1, H, W), new(1, H, W)
    plist = C.c_void_p(0)
    L.check(lib.syn3r_raster_render(N, H, W, bg, L.ptr(radii), L.ptr(geom), geom.numel(), L.ptr(binning), binning.numel(), L.ptr(image),
                                    image.numel(), P, L.ptr(color), L.ptr(depth), L.ptr(alpha), C.byref(plist), stream), "syn3r_raster_render")
    torch.cuda.synchronize(dev)
    return geom[:16].view(torch.int32).cpu().tolist(), P, color


@pytest.mark.parametrize("H,W", TINY_SIZES, ids=[f"{h}x{w}" for h, w in TINY_SIZES])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_geometry_header_is_cleared_whatever_n(N, H, W, gpu):
    """A geometry buffer full of 0xFF through the C ABI: after the two forward stages header[0] is the pair count, header[1] (the
    overflow flag of the async mode) is 0, header[3] (the exact count the binning adds its rectangles' areas INTO) is the pair count
    too and header[2], the entries of the super-tile lists, is at most that."""
    sc = tiny_scene(N, H, W)
    ref = _tiny_reference(sc, "plain")
    pairs = len(ref["aux"]["point_list"])
    header, P, color = _abi_render(sc, gpu, 0xFF)
    assert P == pairs
    assert header[1] == 0, header
    assert header[0] == pairs, header
    assert header[3] == pairs and 0 < header[2] <= pairs, header
    np.testing.assert_allclose(color.cpu().numpy(), ref["color"].numpy(), atol=COLOR_ATOL)


def test_overflow_report_of_a_three_gaussian_scene(gpu, monkeypatch):
    """Capacity forced to 16 where the scene has 46 pairs: the next flush_pair_checks() raises once, the capacity it leaves comes
    from the EXACT pair count (header[3], which the binning accumulates into: garbage there became the next capacity), and one
    re-render is the sync render bit for bit.  Under the three patterns (0xFF is the buffer of the check above)."""
    from syn3r_amd import _lib as L
    from syn3r_amd import raster
    N, H, W = 3, 64, 96
    sc = tiny_scene(N, H, W)
    with torch.no_grad():
        pairs = len(A.rasterize(sc, 3, False)[0][4]["point_list"])
    assert pairs >= 32
    key = raster.capacity_key(gpu, N, H, W)
    for byte in PATTERNS:
        with poisoned(monkeypatch, byte):
            sync = _forward(sc, gpu, 3, "plain")[:4]
            raster.set_pair_count_mode("async")
            try:
                raster._capacity.pop(key, None)
                _forward(sc, gpu, 3, "plain")                         # the first call of the shape sizes exactly
                assert raster.flush_pair_checks() == 0
                raster._capacity[key] = 16
                _forward(sc, gpu, 3, "plain")
                with pytest.raises(L.Syn3rError) as e:
                    raster.flush_pair_checks()
                assert e.value.truncated == 1
                cap = raster._capacity[key]
                assert pairs <= cap <= pairs + int(pairs * raster._HEADROOM) + 4096, (hex(byte), cap, pairs)
                again = _forward(sc, gpu, 3, "plain")[:4]
                assert raster.flush_pair_checks() == 0
            finally:
                raster._pending.clear()
                raster.set_pair_count_mode("sync")
            for a, b in zip(again, sync):
                assert torch.equal(a, b), hex(byte)


# ======================================================================================================== the other ops
# A row of this part runs the op's own test function (tests/test_*_gpu.py: its inputs, its float64 reference, its bars) inside the
# poisoned block, with the public functions it calls wrapped so that every tensor they return is recorded: the recorded tensors are
# the row's outputs (finite check, bit comparison across the patterns), the test function itself is the reference check.
def _flatten(label, x, rec):
    if isinstance(x, np.ndarray):                     # (forward_warp hands numpy arrays back)
        x = torch.from_numpy(np.ascontiguousarray(x).copy())
    if isinstance(x, torch.Tensor):
        rec.append((label, x.detach()))
    elif isinstance(x, (tuple, list)):
        for k, v in enumerate(x):
            _flatten(f"{label}[{k}]", v, rec)
    elif isinstance(x, dict):
        for k in sorted(x, key=str):
            _flatten(f"{label}.{k}", x[k], rec)
    elif hasattr(x, "__dataclass_fields__"):
        for k in x.__dataclass_fields__:
            _flatten(f"{label}.{k}", getattr(x, k), rec)


def _recording(monkeypatch, targets, body):
    """body() with every (object, attribute name) of `targets` wrapped: -> [(label, tensor)] of everything they returned, in order"""
    rec = []
    with monkeypatch.context() as m:
        for obj, name in targets:
            def wrapped(*a, __fn=getattr(obj, name), __name=name, **k):
                out = __fn(*a, **k)
                _flatten(__name, out, rec)
                return out
            m.setattr(obj, name, wrapped)
        body()
    return rec


def recorded_row(name, targets, body, monkeypatch, atomics=(), nonfinite=()):
    """`atomics`: label fragments of outputs that float atomics feed (finite, reference-checked by `body`, not bit-compared);
    `nonfinite`: label fragments of outputs whose reference has NaN / inf entries (`body` compares the finite pattern itself)."""
    def run(dev):
        rec = _recording(monkeypatch, targets(), lambda: body(dev))
        assert rec, f"{name}: nothing was recorded"
        for label, t in rec:
            if t.is_floating_point() and not any(s in label for s in nonfinite):
                assert bool(torch.isfinite(t).all()), f"{name}: {label} is not finite"
        run.labels = [label for label, _ in rec]
        return tuple(t for label, t in rec if not any(s in label for s in atomics))
    return Row(name, run, True, None, lambda outs: tuple(torch.zeros_like(o, dtype=torch.bool) if isinstance(o, torch.Tensor) else None for o in outs))


def _train_ops(*names):
    def targets():
        """each name where the tests find it (the package root) and where its sibling operators do (the module that defines it)"""
        import sys
        from syn3r_amd.gs import train_ops
        return [(where, n) for n in names for where in (train_ops, sys.modules[getattr(train_ops, n).__module__])]
    return targets


def _unet_ops(*names):
    def targets():
        from syn3r_amd.unet import ops
        return [(ops, n) for n in names]
    return targets


# ---------------------------------------------------------------------------------------------- sort_pairs
def _raster_sort():
    from syn3r_amd import raster
    return [(raster, "sort_pairs")]


@pytest.mark.parametrize("nbits", [64, 45])
@pytest.mark.parametrize("n", [1, 4097, 600_000])
def test_sort_pairs_rows(n, nbits, gpu, monkeypatch):
    """600 000 pairs are 147 blocks: past the fused form (128 blocks), inside the single-block scan of 64 items per thread."""
    import test_raster_gpu as TR
    run_row(recorded_row(f"sort_pairs n={n} nbits={nbits}", _raster_sort, lambda dev: TR.test_sort_pairs_matches_stable_sort(n, nbits, dev),
                         monkeypatch), monkeypatch, gpu)


# ---------------------------------------------------------------------------------------------- neighbour search
@pytest.mark.parametrize("kind,n", [("uniform", 4), ("uniform", 1025), ("duplicates", 5000)])
def test_neighbour_search_rows(kind, n, gpu, monkeypatch):
    import test_knn_gpu as TK
    import test_unpool_gpu as TU

    def body(dev):
        TK.test_knn3_matches_bruteforce_bit_exact(kind, n, dev)
        TU.test_graph_matches_bruteforce_bit_exact(kind, n, dev)
        TU.test_unpool_selects_everything(kind, n, dev)
        if n > 4:
            TU.test_unpool_matches_restatement(kind, n, dev)

    run_row(recorded_row(f"knn3 / graph / unpool {kind} {n}", _train_ops("knn3_mean_dist2", "knn3_graph", "proximity_unpool"), body, monkeypatch),
            monkeypatch, gpu)


def test_statistical_outlier_row(gpu, monkeypatch):
    import test_n2_gpu as TN

    def targets():
        from syn3r_amd import pcd
        return [(pcd, "statistical_outlier")]

    run_row(recorded_row("statistical_outlier clusters-13", targets, lambda dev: TN.test_statistical_outlier_vs_oracle(dev, "clusters", 13, 2),
                         monkeypatch), monkeypatch, gpu)


@pytest.mark.parametrize("N", [1, 257])
def test_filter_3d_rows(N, gpu, monkeypatch):
    import test_filter3d_gpu as TF

    def body(dev):
        for C_ in (1, 3):
            TF.test_filter_kernel_vs_float64(N, C_, dev, _no_measurements)

    run_row(recorded_row(f"compute_filter_3D N={N}", _train_ops("compute_filter_3D"), body, monkeypatch), monkeypatch, gpu)


# ---------------------------------------------------------------------------------------------- losses
LOSS_SHAPES = [(1, 5), (1, 16, 16), (3, 37, 53)]        # [C,H,W] ops take the last two; the depth term their H x W
LAMBDA = {(1, 16, 16): 1.0, (3, 37, 53): 0.2}           # the lambda_dssim these shapes have in tests/test_train_ops_gpu.py
_LOSS_OPS = ("l1_loss", "l1_loss_step", "photometric_loss", "photometric_loss_step", "depth_correlation_loss", "depth_correlation_loss_step",
             "image_metrics")


def _larger_first(dev):
    """the `*_step` forms keep their scratch in the workspace cache: a larger shape first, so that the buffer is reused (and, inside
    a poisoned block, holds that call's leftovers where the pattern was)"""
    from syn3r_amd.gs.train_ops import depth_correlation_loss_step, l1_loss_step, photometric_loss_step
    g = torch.Generator().manual_seed(1)
    a, b = torch.rand(3, 64, 96, generator=g).to(dev), torch.rand(3, 64, 96, generator=g).to(dev)
    m = torch.rand(64, 96, generator=g).to(dev)
    l1_loss_step(a, b, 0.3)
    photometric_loss_step(a, b, 0.2, 0.7)
    photometric_loss_step(a, b, 0.2, 0.7, weight_map=m)
    depth_correlation_loss_step(a[:1] + 1.0, b[0], 0.3)


def _loss_bodies(shape):
    import test_depth_loss_gpu as TD
    import test_photo_map_gpu as TP
    import test_train_ops_gpu as TT
    bodies = {"l1": lambda dev: TT.test_l1_loss_forward_backward(shape, dev),
              "depth_corr": lambda dev: TD.test_op_matches_float64_restatement("random", shape[-2:], dev, _no_measurements)}
    if len(shape) == 3:
        lam = LAMBDA[shape]
        bodies.update({
            "l1_map": lambda dev: TP.test_l1_pair_with_a_map(shape, dev, _no_measurements),
            "photometric": lambda dev: TT.test_photometric_loss_vs_published_formula(shape, lam, dev),
            "photometric_step": lambda dev: TT.test_photometric_loss_step_equals_forward_then_backward(shape, lam, dev),
            "photometric_map": lambda dev: [TP.test_photo_map_vs_float64_autograd(shape, lam, kind, dev, _no_measurements) for kind in TP.MAPS],
            "photometric_map_step": lambda dev: TP.test_photo_map_step_equals_forward_then_backward(shape, dev),
            "image_metrics": lambda dev: _image_metrics_body(shape, dev)})
    return bodies


def _image_metrics_body(shape, dev):
    """the definitions and bars of tests/test_trainer_gpu.py::test_checkpoints_pcd_reset_metrics_and_neighbours"""
    from syn3r_amd.gs.train_ops import image_metrics
    from test_train_ops_gpu import _published_ssim
    g = torch.Generator().manual_seed(4)
    a, b = torch.rand(shape, generator=g).to(dev), torch.rand(shape, generator=g).to(dev)
    m = image_metrics(a, b)
    assert abs(float(m[0]) - float(-10 * torch.log10(((a - b) ** 2).mean()))) < 1e-4
    assert abs(float(m[1]) - float(_published_ssim(a.cpu().double(), b.cpu().double()))) < 1e-5


_LOSS_CASES = [(op, shape) for shape in LOSS_SHAPES for op in ("l1", "depth_corr")] + \
              [(op, shape) for shape in LOSS_SHAPES[1:] for op in ("l1_map", "photometric", "photometric_step", "photometric_map",
                                                                  "photometric_map_step", "image_metrics")]


@pytest.mark.parametrize("op,shape", _LOSS_CASES, ids=[f"{op}-{'x'.join(map(str, s))}" for op, s in _LOSS_CASES])
def test_loss_rows(op, shape, gpu, monkeypatch):
    body = _loss_bodies(shape)[op]

    def with_reuse(dev):
        _larger_first(dev)
        body(dev)

    run_row(recorded_row(f"{op} {shape}", _train_ops(*_LOSS_OPS), with_reuse, monkeypatch), monkeypatch, gpu)


# ---------------------------------------------------------------------------------------------- scheduler
@pytest.mark.parametrize("F,h,w", [(3, 8, 8), (14, 9, 7)])
def test_scheduler_rows(F, h, w, gpu, monkeypatch):
    """step_interp with and without the gradient and step_interp_prob_uncertain (tests/test_sched_gpu.py::check_case runs the three).
    The gradient is scaled by a standard deviation whose two sums are float64 atomics: tolerance-only."""
    import test_sched_gpu as TS

    def targets():
        from syn3r_amd.schedulers.scheduling_euler_discrete import EulerDiscreteScheduler
        return [(EulerDiscreteScheduler, "step_interp"), (EulerDiscreteScheduler, "step_interp_prob_uncertain")]

    run_row(recorded_row(f"scheduler F={F} {h}x{w}", targets, lambda dev: TS.test_steps_other_frame_counts_vs_oracle(F, h, w, "float32", dev),
                         monkeypatch, atomics=(".grad",)), monkeypatch, gpu)


# ---------------------------------------------------------------------------------------------- warps
def _warp_targets():
    from syn3r_amd import orchestrator, pcd
    from syn3r_amd.solver_utils import consistency, forward_warp
    return [(forward_warp, "inverse_warp"), (forward_warp, "inverse_warp_batch"), (forward_warp, "forward_warp"),
            (consistency, "consistency_check_with_depth"), (orchestrator, "warp_images_bw_device"), (orchestrator, "fuse_uncertainty_device"),
            (pcd, "flow_cycle_mask")]


def _warp_bodies():
    import test_n2_gpu as TN
    import test_orchestrator_gpu as TO
    import test_warp_gpu as TW
    return {
        "inverse_warp": lambda dev: TW.test_inverse_warp_vs_oracle_and_golden("small", dev, GOLDEN),
        "inverse_warp_batch": lambda dev: TW.test_inverse_warp_batch_matches_single(dev),
        "consistency_check_with_depth": lambda dev: TW.test_reproj_error_vs_oracle_and_golden("small", dev, GOLDEN),
        "forward_warp": lambda dev: TW.test_forward_warp_vs_oracle_and_golden("small", dev, GOLDEN),
        "warp_post": lambda dev: [TO.test_warp_post_matches_host_restatement(2, 40, 72, 5, 9), TO.test_warp_images_bw_device_vs_per_frame_host_loop()],
        "fuse_uncertainty": lambda dev: TO.test_fuse_uncertainty_device_vs_numpy(),
        "flow_cycle_mask": lambda dev: TN.test_flow_cycle_mask_vs_oracle(dev, 5, 7, 2),
    }


@pytest.mark.parametrize("op", ["inverse_warp", "inverse_warp_batch", "consistency_check_with_depth", "forward_warp", "warp_post",
                                "fuse_uncertainty", "flow_cycle_mask"])
def test_warp_rows(op, gpu, monkeypatch):
    """forward_warp splats with float64 atomics (csrc/warp.hip splat4): its image is tolerance-only; the reprojection errors and the
    cycle distances are NaN / inf where the reference's are."""
    assert gpu.index == 0                                   # (tests/test_orchestrator_gpu.py runs on cuda:0)
    body = _warp_bodies()[op]
    atomics = ("forward_warp[0]",) if op == "forward_warp" else ()          # (the image; the mask and the flow are bit-compared)
    run_row(recorded_row(op, _warp_targets, body, monkeypatch, atomics=atomics, nonfinite=("reproj_error", "soft_mask_reproj", "consistency_check_with_depth",
                                                                                          "flow_cycle_mask")), monkeypatch, gpu)


# ---------------------------------------------------------------------------------------------- UNet ops
_UNET_OPS = ("linear", "conv3x3", "tconv3", "groupnorm", "layernorm", "feedforward", "linear_geglu", "attention", "attention_temporal")


def _unet_bodies():
    import test_gn_epilogue_gpu as TG
    import test_unet_ops_gpu as TU
    return {
        "gemm_plain 37x48x192": lambda dev: TU.test_gemm_plain(37, 48, 192, dev),
        "linear split-K": lambda dev: TU.test_linear_split_k(dev),                    # (their split-K workspace is a torch.empty: poisoned)
        "conv3x3 split-K": lambda dev: TU.test_conv3x3_split_k(4, 8, 8, 128, 160, dev),
        "tconv3 split-K": lambda dev: TU.test_tconv3_split_k(dev),
        "groupnorm": lambda dev: TU.test_groupnorm(2, 1000, 64, False, dev),
        "groupnorm two-source": lambda dev: TU.test_groupnorm_two_source(4, 100, 64, 64, True, dev),
        "groupnorm from epilogue partials": lambda dev: TG.test_groupnorm_two_source_from_partials(320, 320, dev),
        "layernorm addvec": lambda dev: [TU.test_layernorm(37, 1280, dev), TU.test_layernorm(257, 200, dev)],
        "feedforward tiled 129x64x128": lambda dev: TU.test_feedforward_tiled_intermediate(129, 64, 128, dev),
        "attention spatial 2x45x2": lambda dev: TU.test_attention_spatial(2, 45, 2, dev),
        "attention temporal 2x3x7x1": lambda dev: TU.test_attention_temporal(2, 3, 7, 1, dev),
    }


@pytest.mark.parametrize("op", ["gemm_plain 37x48x192", "linear split-K", "conv3x3 split-K", "tconv3 split-K", "groupnorm", "groupnorm two-source",
                                "groupnorm from epilogue partials", "layernorm addvec", "feedforward tiled 129x64x128",
                                "attention spatial 2x45x2", "attention temporal 2x3x7x1"])
def test_unet_op_rows(op, gpu, monkeypatch):
    run_row(recorded_row(op, _unet_ops(*_UNET_OPS), _unet_bodies()[op], monkeypatch), monkeypatch, gpu)


# ---------------------------------------------------------------------------------------------- LPIPS
@pytest.mark.parametrize("precision", ["fp16", "fp16x2"])
def test_lpips_rows(precision, gpu, monkeypatch):
    """value and image gradient at 32 x 48 (the 2 x 3 feature map of the last stage is smaller than any tile)"""
    import test_lpips_gpu as TL
    import test_lpips_split_gpu as TLS
    H, W = 32, 48

    def run(dev):
        from syn3r_amd.gs.lpips import LPIPS
        m = LPIPS(precision=precision).init_random(dev, seed=3)
        a, b = TLS.R.images(H, W, H)
        pred = a.to(dev).requires_grad_(True)
        loss = m(pred, b.to(dev))
        (3.0 * loss).backward()
        return loss.detach(), pred.grad

    def check(_outs):
        if precision == "fp16":
            TL.test_lpips_value_and_gradient_vs_oracle(gpu, H, W, _no_measurements)
        else:
            TLS.test_lpips_split_value_and_gradient_vs_oracle(gpu, H, W, _no_measurements)

    run_row(Row(f"lpips {precision} {H}x{W}", run, True, check), monkeypatch, gpu)
