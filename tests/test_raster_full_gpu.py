"""The rasteriser at the BENCHMARK size — 200 000 Gaussians, 1920x1080, P ~ 2.6 M (Gaussian, tile) pairs — against the CPU
restatement (oracle/raster_oracle.py): images and gradients from tests/golden/raster_200k_1080p*.npz (the float64 oracle
run once by oracle/gen_raster_golden.py, ~25 min of CPU), tile lists from the oracle's own preprocess + stable sort run
live (seconds).  This is where the saturation walk-back, the staging batches and the per-half visit lists of the
blend kernels are stressed; the small-scene tests of test_raster_gpu.py cannot reach them.
PARITY UNPINNED against the reference's CUDA rasteriser (source absent): this pins HIP to the restatement.
Edge scenes (run live against the oracle): an opaque front layer (T < 1e-4 after a few splats), more splats in a tile than
one staging batch (128) and than two, and one Gaussian covering the whole frame."""
import numpy as np
import pytest
import torch

from oracle import gen_raster_golden as GG
from oracle import raster_oracle as RO

pytestmark = pytest.mark.gpu


def _render(gpu, m, s, q, o, sh, H, W, bg, requires_grad, debug):
    from syn3r_amd.raster import GaussianRasterizationSettings, GaussianRasterizer
    view, proj, campos, tfx, tfy = RO.look_at_camera(H, W)
    f = lambda t: t.to(gpu, torch.float32).clone().requires_grad_(requires_grad)
    p = [f(m), f(s), f(q), f(o), f(sh)]
    m2 = torch.zeros(m.shape[0], 3, device=gpu, requires_grad=requires_grad)
    st = GaussianRasterizationSettings(H, W, tfx, tfy, torch.tensor(bg, dtype=torch.float32, device=gpu), 1.0, view.to(gpu),
                                       proj.to(gpu), 3, campos.to(gpu), False, debug)
    out = GaussianRasterizer(st)(p[0], m2, p[3], shs=p[4], scales=p[1], rotations=p[2])
    return out, p, m2


@pytest.fixture(scope="module")
def golden(golden_dir):
    path = golden_dir / "raster_200k_1080p.npz"
    if not path.exists():
        pytest.skip("raster_200k_1080p.npz not generated (oracle/gen_raster_golden.py)")
    return GG.load(path)


@pytest.mark.parametrize("mode", ["sync", "async"])
def test_forward_and_backward_match_oracle_at_benchmark_size(mode, golden, gpu):
    from syn3r_amd import raster
    g = golden
    N, H, W, st, off = int(g["N"]), int(g["H"]), int(g["W"]), int(g["stride"]), int(g["offset"])
    m, s, q, o, sh = RO.synthetic_gaussians(N, seed=1234, dtype=torch.float64)
    raster.set_pair_count_mode(mode)
    try:
        if mode == "async":          # first call of a shape sizes exactly; the second runs on the device-side count
            _render(gpu, m, s, q, o, sh, H, W, tuple(g["bg"]), False, False)
        (color, radii, depth, alpha), p, m2 = _render(gpu, m, s, q, o, sh, H, W, tuple(g["bg"]), True, False)
        wc, wd, wa = GG.loss_weights(H, W)
        loss = (color * wc.float().to(gpu)).sum() + (depth * wd.float().to(gpu)).sum() + (alpha * wa.float().to(gpu)).sum()
        loss.backward()
        raster.flush_pair_checks()
    finally:
        raster.set_pair_count_mode("sync")
    sl = (slice(None), slice(off, None, st), slice(off, None, st))
    c, d, a = (t.detach().cpu().numpy() for t in (color, depth, alpha))
    # ---- images: north_star's "within 1e-3 on rendered RGB"; a pixel whose alpha >= 1/255 or T < 1e-4 decision flips
    # between fp32 and fp64 moves by up to ~1/255
    dc = np.abs(c[sl] - g["color"])
    mse = float((dc.astype(np.float64) ** 2).mean())
    psnr = 10 * np.log10(1.0 / max(mse, 1e-30))
    assert psnr > 60.0, psnr
    assert float((dc > 1e-3).mean()) < 1e-4 and float(dc.max()) < 5e-3, (float(dc.max()), float((dc > 1e-3).mean()))
    assert float((np.abs(a[sl] - g["alpha"]) > 1e-3).mean()) < 1e-4
    dd = np.abs(d[sl] - g["depth"])
    assert float((dd > 2e-3).mean()) < 2e-4 and float(dd.max()) < 5e-2, (float(dd.max()), float((dd > 2e-3).mean()))
    # whole-image sums (the stored sample is strided)
    np.testing.assert_allclose(c.astype(np.float64).sum((1, 2)), g["color_sum"], rtol=2e-5)
    np.testing.assert_allclose(float(a.astype(np.float64).sum()), float(g["alpha_sum"]), rtol=2e-5)
    np.testing.assert_allclose(float(d.astype(np.float64).sum()), float(g["depth_sum"]), rtol=2e-5)
    # ---- gradients: sampled Gaussians and per-group sums against float64 autograd through the oracle
    ids = torch.from_numpy(g["sample_ids"])
    for k, t in zip(("m", "s", "q", "o", "sh"), p):
        got = t.grad.detach().cpu().double()
        ref = torch.from_numpy(g[f"grad_{k}_sample"]).double()
        scale = float(g[f"grad_{k}_max"])
        err = (got[ids].reshape(ref.shape) - ref).abs()
        # float atomics + the few flipped threshold decisions: 2e-3 of the group's largest gradient, as at small sizes
        assert float(err.max()) < 2e-3 * scale, (k, float(err.max()), scale)
        assert abs(float(got.abs().sum()) - float(g[f"grad_{k}_abs"])) < 1e-3 * float(g[f"grad_{k}_abs"]), k
        assert abs(float(got.sum()) - float(g[f"grad_{k}_sum"])) < 1e-3 * float(g[f"grad_{k}_abs"]), k
    sg = m2.grad.detach().cpu().double()[ids][:, :2]
    ref = torch.from_numpy(g["screen_grad_sample"]).double()
    # means2D gradient as the published backward defines it: d L / d (NDC mean) = d L / d (pixel mean) * (W/2, H/2)
    ref = ref * torch.tensor([0.5 * W, 0.5 * H], dtype=torch.float64)
    assert float((sg - ref).abs().max()) < 2e-3 * float(ref.abs().max())
    print(f"200k/1080p {mode}: PSNR {psnr:.1f} dB, max |dRGB| {float(dc.max()):.2e}")


def _check_tile_lists(gpu, N, H, W, bg=(0.1, 0.2, 0.3), scale_mult=1.0):
    """The oracle's float32 preprocess + stable sort of the published (tile << 32 | depth bits) keys, run live, against the
    HIP binning.  A Gaussian whose 3-sigma radius lands on an integer boundary may get a different ceil() from the two fp32
    evaluation orders: those (a handful in 200 000) are removed from both lists, everything else must agree index for
    index.  Returns the oracle's ranges."""
    from syn3r_amd.raster import _Rasterize
    m, s, q, o, sh = RO.synthetic_gaussians(N, seed=1234, dtype=torch.float32)
    s = s * scale_mult
    (color, radii, depth, alpha), _, _ = _render(gpu, m, s, q, o, sh, H, W, bg, False, True)
    dbg = _Rasterize.debug_state
    view, proj, campos, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float32)
    pre = RO.preprocess(m, s, q, o, sh, None, view, proj, campos, tfx, tfy, H, W, 3)
    keys, plist, ranges = RO.build_tile_lists(pre)
    valid = pre["valid"].numpy()
    hip_r = radii.cpu().numpy()
    odd = np.nonzero(hip_r != pre["radius"].numpy())[0]
    assert len(odd) < 1e-4 * N + 2, len(odd)
    # depths agree bit for bit on the Gaussians both sides render
    both = valid & (hip_r > 0)
    np.testing.assert_array_equal(dbg["depths"].cpu().numpy()[both], pre["depth"].numpy()[both])
    hp = dbg["point_list"].cpu().numpy().astype(np.int64)
    hr = dbg["ranges"].cpu().numpy().astype(np.int64)
    if len(odd) == 0:
        assert dbg["num_rendered"] == len(plist)
        np.testing.assert_array_equal(hp, plist)
        np.testing.assert_array_equal(hr, ranges)
    else:
        def per_tile(pl, rg):
            tile_of = np.repeat(np.arange(len(rg)), np.maximum(rg[:, 1] - rg[:, 0], 0))
            keep = ~np.isin(pl, odd)
            return pl[keep], tile_of[keep]
        assert abs(dbg["num_rendered"] - len(plist)) <= 64 * len(odd)
        a_ids, a_tiles = per_tile(hp, hr)
        b_ids, b_tiles = per_tile(plist, ranges)
        np.testing.assert_array_equal(a_ids, b_ids)          # same Gaussians in the same order ...
        np.testing.assert_array_equal(a_tiles, b_tiles)      # ... in the same tiles
    print(f"tile lists {N} @ {W}x{H}: P = {dbg['num_rendered']}, {len(odd)} Gaussians with a ceil() tie excluded")
    return ranges


def test_tile_lists_index_for_index_at_benchmark_size(golden, gpu):
    """north_star: 'bit-exact on tile/sort indices' at P ~ 2.6 M pairs."""
    _check_tile_lists(gpu, int(golden["N"]), int(golden["H"]), int(golden["W"]), tuple(golden["bg"]))


@pytest.mark.parametrize("N,H,W,scale,what", [
    (300_000, 1080, 1920, 1.0, "two rounds per binning block (more than 65 536 / 135 chunks of 512 Gaussians)"),
    (60_000, 2160, 3840, 1.0, "510 super-tiles: eight mask words per wavefront, one column part per thread"),
    (20_000, 1152, 8192, 1.0, "576 super-tiles: beyond the hierarchical binning, the pair sort takes it"),
    (5_000, 100, 260, 1.0, "ragged image: partial tiles and partial super-tiles on both edges"),
    (4_000, 1080, 1920, 10.0, "large footprints: more list entries per block round than the LDS staging holds"),
    (20_000, 48, 40, 1.0, "nine single-tile super-tiles, lists of 155 .. 15 487: k_super_sort in LDS, in 3 pieces and in 4 (the last partial)"),
])
def test_tile_lists_other_binning_shapes(N, H, W, scale, what, gpu):
    """The hierarchical binning (csrc/raster_bin.hip: super-tile lists, then a filter per tile) and its fallback at the shapes
    that take its other branches; same oracle, same index-for-index bar."""
    ranges = _check_tile_lists(gpu, N, H, W, scale_mult=scale)
    if (H, W) == (48, 40):
        # k_super_sort orders up to kSortLds = 4096 keys in LDS and longer lists in LDS-sized pieces merged through global memory
        # (the 8 192 merge, and the 16 384 merge with its distance-4096 global step): the scene must stay on both sides of that
        lens = ranges[:, 1] - ranges[:, 0]
        assert int(lens.max()) > 8192, lens
        assert bool(((lens > 0) & (lens <= 4096)).any()), lens


def _edge_scene(kind, N, H, W):
    dt = torch.float64
    g = torch.Generator().manual_seed(17)
    m = torch.stack([(torch.rand(N, generator=g, dtype=dt) * 2 - 1) * 0.02, (torch.rand(N, generator=g, dtype=dt) * 2 - 1) * 0.02,
                     3.0 + torch.rand(N, generator=g, dtype=dt)], 1)
    s = torch.full((N, 3), 0.004, dtype=dt)
    q = torch.zeros(N, 4, dtype=dt); q[:, 0] = 1
    o = torch.full((N,), 0.05, dtype=dt)
    sh = 0.3 * torch.randn(N, 16, 3, generator=g, dtype=dt)
    if kind == "opaque_front":        # a few large, nearly opaque Gaussians in front: T < 1e-4 after three of them
        m[:6, 2] = 2.0 + 0.01 * torch.arange(6, dtype=dt)
        s[:6] = 2.0
        o[:6] = 0.98          # alpha < 0.99 (no clamp): T = 0.02^k never sits ON the 1e-4 threshold
    elif kind == "whole_frame":       # one Gaussian whose 3-sigma footprint covers every tile
        m[0] = torch.tensor([0.0, 0.0, 2.5], dtype=dt)
        s[0] = 3.0
        o[0] = 0.6
    return m, s, q, o, sh


@pytest.mark.parametrize("kind,N", [("opaque_front", 300), ("deep_tile", 140), ("deep_tile", 700), ("whole_frame", 200)])
def test_edge_scenes_vs_oracle(kind, N, gpu):
    """'deep_tile': every Gaussian lands in the same few tiles, so a tile's list is longer than one staging batch of the
    blend kernels (128) / than several, with low opacities so that no pixel saturates early."""
    H, W = 48, 80
    m, s, q, o, sh = _edge_scene(kind, N, H, W)
    bg = (0.2, 0.1, 0.4)
    (color, radii, depth, alpha), p, _ = _render(gpu, m, s, q, o, sh, H, W, bg, True, True)
    from syn3r_amd.raster import _Rasterize
    dbg = _Rasterize.debug_state
    view, proj, campos, tfx, tfy = RO.look_at_camera(H, W, dtype=torch.float64)
    op = [t.clone().requires_grad_(True) for t in (m, s, q, o, sh)]
    oc, orad, od, oa, aux = RO.rasterize(op[0], op[1], op[2], op[3], op[4], None, view, proj, campos, tfx, tfy, H, W,
                                         torch.tensor(bg, dtype=torch.float64), 3)
    longest = int((aux["ranges"][:, 1] - aux["ranges"][:, 0]).max())
    if kind == "deep_tile":
        assert longest > (128 if N < 300 else 512), longest
    if kind == "whole_frame":
        assert int((aux["ranges"][:, 1] > aux["ranges"][:, 0]).sum()) == aux["ranges"].shape[0]       # every tile is touched
    if kind == "opaque_front":
        assert int(aux["n_contrib"].max()) <= 6 and float(oa.min()) > 0.99                               # saturates within the front layer
    np.testing.assert_array_equal(dbg["point_list"].cpu().numpy(), aux["point_list"])
    np.testing.assert_array_equal(dbg["ranges"].cpu().numpy(), aux["ranges"])
    assert (dbg["n_contrib"].cpu().numpy() != aux["n_contrib"]).mean() < 2e-3
    np.testing.assert_allclose(color.detach().cpu().numpy(), oc.detach().numpy(), atol=3e-4)
    np.testing.assert_allclose(alpha.detach().cpu().numpy(), oa.detach().numpy(), atol=3e-4)
    np.testing.assert_allclose(depth.detach().cpu().numpy(), od.detach().numpy(), atol=2e-3, rtol=1e-4)
    gen = torch.Generator().manual_seed(5)
    wc = torch.randn(3, H, W, generator=gen, dtype=torch.float64)
    wa = torch.randn(1, H, W, generator=gen, dtype=torch.float64)
    ((color * wc.float().to(gpu)).sum() + (alpha * wa.float().to(gpu)).sum()).backward()
    ((oc * wc).sum() + (oa * wa).sum()).backward()
    for k, a_, b_ in zip("msqoh", p, op):
        scale = float(b_.grad.abs().max()) + 1e-12
        err = float((a_.grad.cpu().double() - b_.grad).abs().max()) / scale
        assert err < 3e-3, (kind, k, err, scale)
