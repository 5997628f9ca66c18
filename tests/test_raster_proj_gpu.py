"""The projection stage of the rasteriser on the HIP path - k_preprocess<AA,F3D>, k_preprocess_bwd<STAGED,AA,F3D,false> with
sh_backward, and what they share in csrc/raster_common.h - PER GAUSSIAN against the float64 reference of tests/raster_proj_ref.py
(scenes, measure, bars and mutants are explained there; tests/test_raster_proj_cpu.py shows that the bars catch the mutants).

Forward: one render through the C ABI (tests/raster_direct.py), the geometry state decoded with carve_geom's layout.  Backward: the
Python surface (`rasterize_forward` / `rasterize_backward`) on the activated and the raw route, under both losses, with every buffer
the surface allocates poisoned (tests/poison.py, 0xFF = NaN): a culled Gaussian's exact zeros are zeros the kernel WROTE.

MEASURED on an MI355X: the worst per-Gaussian rel of each family and group over all its cases (both losses; the
`measurements` fixture records one "raster_proj_backward" line per case).  raster_proj_ref.BAR holds <= 2 x these.
    family    m        s        q        q_raw    o        sh       cf       m2
    lattice   9.98e-6  1.37e-6  1.55e-6  2.59e-5  1.56e-6  7.94e-7  1.53e-6  1.09e-5
    layouts   3.66e-5  5.93e-6  7.17e-6  -        6.30e-6  5.06e-7  6.29e-6  3.58e-5
    guard     1.59e-6  1.32e-6  1.67e-6  9.08e-6  1.75e-6  1.70e-6  1.73e-6  1.57e-6
    blocks    2.43e-6  8.58e-7  1.45e-6  -        1.33e-6  5.06e-7  1.37e-6  2.86e-6
    near      1.88e-5  1.27e-5  1.27e-5  -        8.19e-7  5.77e-7  7.88e-7  1.38e-5
Where the worst cases sit: lattice m / m2 under both filters (f3d_aa), q_raw at quaternion norm 1e-3 (2.59e-5) and 1e3 (2.24e-5) under
f3d_aa, against 4.5e-6 at the norms 0.5 and 2 without a filter; layouts: every group but sh at degree 0 with one coefficient under the
colour-only loss; guard: the controls just inside the band, q_raw under f3d; near: s and q are the regulariser's 1.2e-5.  The staged
(16-byte aligned) and the unstaged (misaligned) kernel at 16 coefficients meet the same bars; their gradients of o and cf are the same
bits, the others differ in the last bits (recorded as "raster_proj_misaligned_bits").
Forward (bounds from the arithmetic, raster_proj_ref.FWD_BAR; measured worst over every case): depth 0 (the view matrix is the
identity), means2D 7.7e-6 px, cov3D 6.7e-7, conic 8.4e-7, rgb 1.1e-7, blend opacity 2.4e-7, opacity 0 (activated) / 7.1e-8 (raw).
Two runs of the suite gave the same figures to three digits everywhere but guard q_raw (8.02e-6 and 9.08e-6: a footprint of many
tiles, whose atomic sums change order); profiles/r23/raster_projection_tests.txt has both, and what the tests do against a library
with four of the mutants compiled into the kernels.
"""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_proj_ref as P  # noqa: E402
from poison import poisoned  # noqa: E402
from raster_direct import render_direct  # noqa: E402

pytestmark = pytest.mark.gpu

LOSSES = ("full", "colour")
MODE_IDS = list(P.MODES)


def f32(t, dev):
    return t.to(torch.float32).to(dev).contiguous()


# ------------------------------------------------------------------------------------------------------------------ forward
def _a256(x):
    return (x + 255) & ~255


def decode_geometry(geometry, N):
    """Direct.geometry -> its arrays, by carve_geom's layout (csrc/raster_fwd.hip): a 256-byte header, then depths [N], means2D [N,2],
    cov3D [N,6], conic_opacity [N,4], rgb [N,3], clamped [N], tiles_touched [N], point_offsets [N], splats [N] x 48 bytes, each
    array 256-byte aligned"""
    out, off = {}, 256
    for name, width, dtype in (("depths", 1, torch.float32), ("means2D", 2, torch.float32), ("cov3D", 6, torch.float32),
                               ("conic_opacity", 4, torch.float32), ("rgb", 3, torch.float32), ("clamped", 1, torch.int32),
                               ("tiles_touched", 1, torch.int32), ("point_offsets", 1, torch.int32), ("splats", 12, torch.float32)):
        out[name] = geometry[off:off + 4 * width * N].view(dtype).reshape(N, width).cpu()
        off += _a256(4 * width * N)
    assert off == geometry.numel()
    return out


def check_forward(sc, dev, deg, mode, measurements, sm=1.0, conf=True, raw=False):
    """one render of `sc` through syn3r_raster_preprocess_f3d / syn3r_raster_render; every per-Gaussian value of the projection
    against the float64 reference.  With `raw` the parameters are raster_f3d_ref.raw_params(sc) (render_direct forms them)."""
    from syn3r_amd import _lib as L
    aa, f3d = P.MODES[mode]
    scene = dict(sc) if conf else dict(sc, cf=None)
    rawp = {k: t for k, t in P.raw_params(sc).items()} if raw else None
    ref = P.reference(sc, deg, mode, "full", sm=sm, conf=conf, raw=rawp, tag=None)
    d = render_direct(L.load(), scene, dev, deg, "f3d", raw=int(raw), flags=L.RASTER_ANTIALIAS if aa else 0,
                      filter3d=f32(sc["f"], dev) if f3d else None, scale_modifier=sm)
    N = sc["N"]
    g = decode_geometry(d.geometry, N)
    radii = d.radii.cpu().to(torch.int64)
    vis = ref["valid"]
    # exact: radii, the culled set, tiles_touched, the clamp mask
    assert torch.equal(radii > 0, vis), "culled set"
    assert torch.equal(radii, ref["radius"]), (radii[vis], ref["radius"][vis])
    assert torch.equal(g["tiles_touched"][:, 0].to(torch.int64), ref["tiles_touched"])
    assert torch.equal(g["clamped"][vis, 0].to(torch.int64), ref["clamped"][vis])
    # the Splat record holds the separately stored values bit for bit (x, y, cxx, cxy, cyy, opacity, r, g, b, depth, 0, 0)
    sp = g["splats"][vis]
    assert torch.equal(sp[:, 0:2], g["means2D"][vis]) and torch.equal(sp[:, 2:5], g["conic_opacity"][vis, :3])
    assert torch.equal(sp[:, 6:9], g["rgb"][vis]) and torch.equal(sp[:, 9:10], g["depths"][vis]) and bool((sp[:, 10:] == 0).all())
    own = lambda got, want: float(((got.double() - want).abs().amax(1) / want.abs().amax(1))[vis].max())
    err = dict(depth=own(g["depths"], ref["depth"][:, None]),
               means2D=float((g["means2D"].double() - ref["means2D"]).abs()[vis].max()),
               cov3D=own(g["cov3D"], ref["cov3D"]), conic=own(g["conic_opacity"][:, :3], ref["conic"]),
               rgb=float((g["rgb"].double() - ref["rgb"]).abs()[vis].max()),
               blend_opacity=own(g["splats"][:, 5:6], ref["blend_opacity"][:, None]),
               opacity=own(g["conic_opacity"][:, 3:4], ref["opacity"][:, None]))
    print(sc["name"], mode, f"sm={sm} conf={conf} raw={raw}", {k: f"{v:.2e}" for k, v in err.items()})
    measurements("raster_proj_forward", scene=sc["name"], mode=mode, sm=sm, conf=conf, raw=raw, visible=int(vis.sum()), **err)
    if not raw:
        assert err["opacity"] == 0.0          # the activated route stores the opacity it was given
    for k, v in err.items():
        assert v <= P.FWD_BAR[k], (k, v)
    return d, ref


@pytest.mark.parametrize("mode", MODE_IDS)
def test_forward_lattice(mode, gpu, measurements):
    lat = P.lattice()
    for conf in (True, False):
        for raw in (False, True):
            check_forward(lat, gpu, 3, mode, measurements, conf=conf, raw=raw)
    for sm in (0.5, 2.0):
        check_forward(P.with_modifier(lat, sm), gpu, 3, mode, measurements, sm=sm)


@pytest.mark.parametrize("mode", MODE_IDS)
def test_forward_guard(mode, gpu, measurements):
    for which in P.GUARD:
        check_forward(P.guard(which), gpu, 3, mode, measurements)


def test_forward_clamp_and_sh_layouts(gpu, measurements):
    d, ref = check_forward(P.clamp_scene(), gpu, 3, "plain", measurements)
    assert ref["clamped"].tolist() == list(range(8))
    for deg, M in P.SH_LAYOUTS:
        check_forward(P.with_coeffs(P.lattice(), M), gpu, deg, "plain", measurements)


@pytest.mark.parametrize("N", P.BLOCK_N)
def test_forward_blocks(N, gpu, measurements):
    check_forward(P.blocks(N), gpu, 3, "plain", measurements)


def test_forward_near_plane(gpu, measurements):
    """the pairs on either side of kNearClip, and the Gaussian exactly AT float32(0.2): `t.z <= kNearClip` culls it (the culled set
    is compared exactly; a `<` keeps it, tests/test_raster_proj_cpu.py::test_mutant_near_lt_is_caught_by_the_culled_set)"""
    d, ref = check_forward(P.near_scene(), gpu, 3, "plain", measurements)
    assert (d.radii.cpu() > 0).tolist() == [False, True] * 4 + [False]


# ------------------------------------------------------------------------------------------------------------------ backward
def hip_grads(sc, dev, deg, mode, loss, monkeypatch, sm=1.0, conf=True, raw=None, shs=None):
    """the gradients of `loss` from the Python surface, every buffer it allocates poisoned with NaN bytes -> ({group: tensor}, radii)"""
    from syn3r_amd.raster import GaussianRasterizationSettings, rasterize_backward, rasterize_forward
    aa, f3d = P.MODES[mode]
    p = raw if raw is not None else sc
    st_ = GaussianRasterizationSettings(P.H, P.W, sc["tfx"], sc["tfy"], f32(sc["bg"], dev), float(sm), f32(sc["view"], dev),
                                        f32(sc["proj"], dev), deg, f32(sc["campos"], dev), False, False, aa)
    args = (f32(sc["m"], dev), shs if shs is not None else f32(sc["sh"], dev), f32(p["o"], dev), f32(p["s"], dev), f32(p["q"], dev),
            f32(sc["cf"], dev) if conf else None)
    flt = f32(sc["f"], dev) if f3d else None
    wc, wd, wa = (f32(w, dev) if w is not None else None for w in P.loss_weights(loss))
    with poisoned(monkeypatch, 0xFF), torch.no_grad():
        _, radii, _, _, st = rasterize_forward(*args, st_, raw_params=raw is not None, filter_3D=flt)
        d_m3, d_m2, d_sh, d_op, d_sc, d_ro, d_cf = rasterize_backward(st, wc, wd, wa)
        torch.cuda.synchronize(dev)
    assert shs is None or (st.shs.data_ptr() == shs.data_ptr() and shs.data_ptr() % 16 == 4)
    got = dict(m=d_m3, s=d_sc, q=d_ro, o=d_op, sh=d_sh, m2=d_m2)
    if conf:
        got["cf"] = d_cf
    return {k: v.cpu() for k, v in got.items()}, radii.cpu().to(torch.int64), st


def check_backward(sc, dev, deg, mode, monkeypatch, measurements, family, sm=1.0, conf=True, raw=None, tag=None, shs=None,
                   losses=LOSSES):
    """both losses: rel[k][i] < BAR[family][k] for every visible Gaussian i and every group k, every culled Gaussian's outputs exactly
    zero (NaN-poisoned buffers), dL_dmeans2D's third column zero.  -> {loss: ({group: tensor}, reference)}"""
    out = {}
    for loss in losses:
        ref = P.reference(sc, deg, mode, loss, sm=sm, conf=conf, raw=raw, tag=tag)
        got, radii, _ = hip_grads(sc, dev, deg, mode, loss, monkeypatch, sm=sm, conf=conf, raw=raw, shs=shs)
        vis = ref["valid"]
        assert torch.equal(radii, ref["radius"])
        worst, at = {}, {}
        for k, t in got.items():
            want = ref["grads_raw"][k] if raw is not None and k in ref["grads_raw"] else ref["grads"][k]
            assert bool(torch.isfinite(t).all()), (k, "not finite: a value nobody wrote, or a NaN of the kernel's")
            assert float(t[~vis].abs().sum()) == 0.0, (k, "a culled Gaussian's gradient is not zero")
            rel, _ = P.per_gaussian(k, t, want)
            rel = torch.where(vis, rel, torch.zeros_like(rel))
            k = "q_raw" if raw is not None and k == "q" else k          # a bar of its own (raster_proj_ref.BAR)
            worst[k], at[k] = float(rel.max()), int(rel.argmax())
        assert float(got["m2"][:, 2].abs().sum()) == 0.0
        print(sc["name"], mode, loss, f"sm={sm} conf={conf} raw={tag if raw is not None else False}",
              {k: f"{v:.2e}@{at[k]}" for k, v in worst.items()})
        measurements("raster_proj_backward", family=family, scene=sc["name"], mode=mode, loss=loss, sm=sm, conf=conf,
                     raw=(str(tag) if raw is not None else None), misaligned=shs is not None, **worst)
        for k, v in worst.items():
            assert v < P.BAR[family][k], (sc["name"], mode, loss, k, v, at[k])
        out[loss] = (got, ref)
    return out


@pytest.mark.parametrize("mode", MODE_IDS)
def test_backward_lattice(mode, gpu, monkeypatch, measurements):
    """with and without the confidence; activated and raw route (raster_f3d_ref.raw_params: quaternion norms in [0.5, 2])"""
    lat = P.lattice()
    for conf in (True, False):
        check_backward(lat, gpu, 3, mode, monkeypatch, measurements, "lattice", conf=conf)
    check_backward(lat, gpu, 3, mode, monkeypatch, measurements, "lattice", raw=P.raw_params(lat), tag="f3d_ref")


@pytest.mark.parametrize("k", P.RAW_NORMS)
def test_backward_raw_quaternion_norms(k, gpu, monkeypatch, measurements):
    lat = P.lattice()
    check_backward(lat, gpu, 3, "f3d_aa", monkeypatch, measurements, "lattice", raw=P.raw_params(lat, k), tag=k)
    check_backward(lat, gpu, 3, "plain", monkeypatch, measurements, "lattice", raw=P.raw_params(lat, k), tag=k, losses=("full",))


@pytest.mark.parametrize("sm", [0.5, 2.0])
@pytest.mark.parametrize("mode", MODE_IDS)
def test_backward_scale_modifier(mode, sm, gpu, monkeypatch, measurements):
    sc = P.with_modifier(P.lattice(), sm)
    check_backward(sc, gpu, 3, mode, monkeypatch, measurements, "lattice", sm=sm)
    check_backward(sc, gpu, 3, mode, monkeypatch, measurements, "lattice", sm=sm, raw=P.raw_params(sc), tag="f3d_ref", losses=("full",))


@pytest.mark.parametrize("mode", MODE_IDS)
def test_backward_guard(mode, gpu, monkeypatch, measurements):
    """beyond the kFovGuard band (x_mul / y_mul zero dtx / dty, ewa_rows clamps tx / ty), in both axes and signs, and just inside it"""
    for which in P.GUARD:
        sc = P.guard(which)
        check_backward(sc, gpu, 3, mode, monkeypatch, measurements, "guard")
        check_backward(sc, gpu, 3, mode, monkeypatch, measurements, "guard", raw=P.raw_params(sc), tag="f3d_ref", losses=("full",))


def test_backward_clamp(gpu, monkeypatch, measurements):
    """clamp masks 0 .. 7: the gradients of a clamped channel's SH coefficients are exactly 0, the others meet the bar"""
    sc = P.clamp_scene()
    for loss, (got, ref) in check_backward(sc, gpu, 3, "plain", monkeypatch, measurements, "lattice").items():
        for k in range(8):
            for c in range(3):
                assert (float(got["sh"][k, :, c].abs().max()) == 0.0) == bool((k >> c) & 1), (loss, k, c)


def misaligned_like(t):
    """the values of `t` in storage that starts one float into a larger buffer: 4-byte, not 16-byte aligned"""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@pytest.mark.parametrize("deg,M", P.SH_LAYOUTS)
def test_backward_sh_layouts(deg, M, gpu, monkeypatch, measurements):
    """every (degree, coefficients) pair; with 16 coefficients the staged kernel (PRELOAD reads all 48 floats, the tail loop zeroes the
    rows from (degree + 1)^2 on) AND, with the SH storage one float off a 16-byte boundary, the unstaged one"""
    sc = P.with_coeffs(P.lattice(), M)
    runs = [check_backward(sc, gpu, deg, "plain", monkeypatch, measurements, "layouts")]
    if M == 16:
        runs.append(check_backward(sc, gpu, deg, "plain", monkeypatch, measurements, "layouts", shs=misaligned_like(f32(sc["sh"], gpu))))
    for run in runs:
        for loss, (got, ref) in run.items():
            assert got["sh"].shape == (sc["N"], M, 3)
            assert float(got["sh"][:, (deg + 1) ** 2:].abs().sum()) == 0.0
            assert bool((got["sh"][:, :(deg + 1) ** 2].abs().amax(dim=(0, 2)) > 0).all())
    if M == 16:          # recorded, not asserted: the blend backward's atomics reorder sums between two launches
        same = {k: torch.equal(runs[0]["full"][0][k], runs[1]["full"][0][k]) for k in runs[0]["full"][0]}
        print("misaligned == aligned, bit for bit:", same)
        measurements("raster_proj_misaligned_bits", deg=deg, **{k: bool(v) for k, v in same.items()})


@pytest.mark.parametrize("N", P.BLOCK_N)
def test_backward_blocks(N, gpu, monkeypatch, measurements):
    """the staged SH path at its block edges: a last block of 1, 255 and 256 rows and of one row behind two full blocks; visible
    Gaussians at a block's first and last rows, every other row a culled one (four kinds) that writes zeros into its LDS row"""
    check_backward(P.blocks(N), gpu, 3, "plain", monkeypatch, measurements, "blocks")


def test_backward_near_plane(gpu, monkeypatch, measurements):
    """point-like Gaussians just beyond the near plane meet the bar of their own (raster_proj_ref.BAR["near"] says why); their
    partners just in front of it, and the one exactly at it, have all-zero gradients"""
    sc = P.near_scene()
    for loss, (got, ref) in check_backward(sc, gpu, 3, "plain", monkeypatch, measurements, "near").items():
        for k, t in got.items():
            assert float(t[[0, 2, 4, 6, 8]].abs().sum()) == 0.0 and float(t[[1, 3, 5, 7]].abs().reshape(4, -1).amax(1).min()) > 0.0, k
