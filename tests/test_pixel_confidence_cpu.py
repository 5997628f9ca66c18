"""`--pixel_confidence` without a GPU: the pure helper that turns the fused uncertainty into per-pixel confidence maps, the flag,
the camera's shape check and `densify_views`' bookkeeping of the maps (an extension: the reference weights a pseudo-view by one
scalar)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch


def test_confidence_maps_from_uncertainty_on_cpu_tensors():
    from syn3r_amd.orchestrator import confidence_maps_from_uncertainty
    g = torch.Generator().manual_seed(0)
    unc = torch.rand(5, 48, 64, generator=g) * 1.6 - 0.3                  # leaves [0,1] on both sides: the clamp acts
    maps = confidence_maps_from_uncertainty(unc, 18, 32)
    assert len(maps) == 7 and maps[0] is None and maps[-1] is None
    ref = torch.nn.functional.interpolate(unc[None], size=(18, 32), mode="bilinear", align_corners=False)[0]
    assert float(ref.max()) > 1.0 and float(ref.min()) < 0.0
    for k, m in enumerate(maps[1:-1]):
        assert m.shape == (18, 32) and m.dtype == torch.float32 and m.is_contiguous()
        assert float(m.min()) >= 0.0 and float(m.max()) <= 1.0
        assert torch.equal(m, (1.0 - ref[k]).clamp(0.0, 1.0))
    assert float(torch.stack(maps[1:-1]).min()) == 0.0 and float(torch.stack(maps[1:-1]).max()) == 1.0
    # the same resolution: 1 - unc itself; no inner frame: the two end frames
    same = confidence_maps_from_uncertainty(unc.clamp(0, 1), 48, 64)
    assert torch.equal(same[2], 1.0 - unc[1].clamp(0, 1))
    assert confidence_maps_from_uncertainty(torch.zeros(0, 8, 8), 4, 4) == [None, None]
    with pytest.raises(ValueError):
        confidence_maps_from_uncertainty(torch.zeros(8, 8), 4, 4)
    assert not unc.requires_grad and unc.min() < 0                         # the input is left alone
    # an undefined (NaN) uncertainty is confidence 0 wherever the resize touches it, and every map stays finite
    holes = unc.clamp(0, 1)
    holes[1, 10:20, 30:40] = float("nan")
    hm = confidence_maps_from_uncertainty(holes, 18, 32)[1:-1]
    href = torch.nn.functional.interpolate(holes[None], size=(18, 32), mode="bilinear", align_corners=False)[0]
    assert bool(href[1].isnan().any()) and all(bool(torch.isfinite(m).all()) for m in hm)
    assert bool((hm[1][href[1].isnan()] == 0).all())
    assert torch.equal(hm[1][~href[1].isnan()], (1.0 - href[1]).clamp(0, 1)[~href[1].isnan()]) and torch.equal(hm[0], 1.0 - href[0])


def test_launcher_flag():
    from syn3r_amd import launch
    assert launch.parse(["--scenes", "x"]).pixel_confidence == 0
    assert launch.parse(["--scenes", "x", "--pixel_confidence", "1"]).pixel_confidence == 1
    for bad in (["--pixel_confidenc", "1"], ["--pixel_confidence", "2"]):
        with pytest.raises(SystemExit):
            launch.parse(["--scenes", "x"] + bad)


def test_camera_checks_the_map_shape():
    from syn3r_amd.gs import Camera
    K = np.array([[40.0, 0, 16], [0, 40.0, 12], [0, 0, 1]], dtype=np.float32)
    mk = lambda **kw: Camera.from_w2c(np.eye(4, dtype=np.float32), K, 24, 32, image=torch.rand(3, 24, 32), data_device="cpu", **kw)
    assert mk().confidence_map is None
    cam = mk(confidence_map=np.full((1, 24, 32), 0.25))
    assert cam.confidence_map.shape == (24, 32) and cam.confidence_map.dtype == torch.float32
    assert float(cam.confidence_map.min()) == 0.25
    for shape in [(32, 24), (3, 24, 32), (24,), (23, 32)]:
        with pytest.raises(ValueError):
            mk(confidence_map=torch.zeros(shape))
        with pytest.raises(ValueError):
            cam.confidence_map = torch.zeros(shape)
    assert cam.confidence_map.shape == (24, 32)                          # a refused map leaves the old one
    cam.confidence_map = None
    assert cam.confidence_map is None
    cam2 = Camera.from_w2c(np.eye(4, dtype=np.float32), K, 24, 32, data_device="cpu", confidence_map=torch.ones(24, 32))
    assert cam2.confidence_map.shape == (24, 32)                         # a camera without an image knows its size too


def _poses(n):
    out = []
    for k in range(n):
        p = np.eye(4, dtype=np.float32)
        p[0, 3] = 0.1 * k
        out.append(p)
    return out


def _densify(tmp_path, flag, dtype="interpolate_gs_v2", rate=1, V=3, with_maps=True):
    """DiffusionGS.densify_views on stand-ins (tests/test_n2_cpu.py's way): frame k of pair i is filled with 100 i + k, and so is
    its map"""
    from syn3r_amd.diffusionGS import DiffusionGS
    me = SimpleNamespace(num_input_views=V, save_dir=str(tmp_path), fps_keyframe_sampling=0, device="cpu",
                         args=SimpleNamespace(pixel_confidence=flag) if flag is not None else SimpleNamespace())

    def interp(i, j, replace=True, perturb_interp_poses=False):
        me._pair_confidence_maps = ([None] + [torch.full((4, 6), 100.0 * i + k) for k in range(1, 24)] + [None]) if with_maps else None
        return [torch.full((3, 4, 6), 100.0 * i + k) for k in range(25)], _poses(25), None

    me._interpolate_between_gs_v3 = interp
    views, poses, pcds = DiffusionGS.densify_views(me, 0, down_sample_rate=rate, densify_type=dtype, num_views_for_pcd_densification=1)
    return me, views


def _ids(maps):
    return [None if m is None else float(m[0, 0]) for m in maps]


def test_densify_views_keeps_maps_parallel_to_the_frames(tmp_path):
    me, views = _densify(tmp_path / "a", 1)
    assert len(views) == 72 and len(me.dense_confidence_maps) == 72
    assert _ids(me.dense_confidence_maps) == [None if k == 0 else 100.0 * i + k for i in range(3) for k in range(24)]
    assert [float(v[0, 0, 0]) for v in views] == [100.0 * i + k for i in range(3) for k in range(24)]
    data = torch.load(tmp_path / "a" / "dense_viewsinterpolated_dense_views_cyc0_view1.pt", weights_only=False)
    assert sorted(data) == ["confidence_maps", "poses", "views"]
    assert _ids(data["confidence_maps"]) == [None] + [100.0 + k for k in range(1, 24)] + [None]
    # a second call reloads the maps from the caches (the stand-in would now hand out none)
    me2, _ = _densify(tmp_path / "a", 1, with_maps=False)
    assert _ids(me2.dense_confidence_maps) == _ids(me.dense_confidence_maps)
    # a cache written without the key loads as all None
    path = tmp_path / "a" / "dense_viewsinterpolated_dense_views_cyc0_view1.pt"
    torch.save({"views": data["views"], "poses": data["poses"]}, path)
    me3, _ = _densify(tmp_path / "a", 1, with_maps=False)
    assert _ids(me3.dense_confidence_maps)[24:48] == [None] * 24 and _ids(me3.dense_confidence_maps)[:24] == _ids(me.dense_confidence_maps)[:24]


def test_densify_views_maps_follow_downsampling_and_the_open_chain(tmp_path):
    me, views = _densify(tmp_path, 1, dtype="interpolate_loop0_gs", rate=0.5)
    idx = list(np.linspace(0, 24, 12, dtype=int))
    want = [100.0 * i + k for i in range(2) for k in idx[:-1]] + [100.0 + 24]
    assert [float(v[0, 0, 0]) for v in views] == want
    assert _ids(me.dense_confidence_maps) == [None if (w % 100) in (0, 24) else w for w in want]


@pytest.mark.parametrize("flag", [0, None])
def test_without_the_flag_nothing_is_kept(flag, tmp_path):
    me, views = _densify(tmp_path, flag)
    assert len(views) == 72 and me.dense_confidence_maps is None
    data = torch.load(tmp_path / "dense_viewsinterpolated_dense_views_cyc0_view0.pt", weights_only=False)
    assert sorted(data) == ["poses", "views"]
