"""One render through the rasteriser's C ABI itself (no Python surface), for the GPU tests that compare the entry families of
include/syn3r_hip.h with each other, and the half-tile masks under which two backward launches give the same bits.  A plain module:
no fixtures, nothing collected."""
import ctypes as C
from typing import Callable, NamedTuple

import torch

import raster_f3d_ref as F

# family -> (suffix of syn3r_raster_preprocess / syn3r_raster_backward, does the entry take raw and flags, does it take a filter)
FAMILIES = {"plain": ("", False, False), "raw": ("_raw", False, False), "ex": ("_ex", True, False), "f3d": ("_f3d", True, True)}


def half_tile_masks(H, W, dev):
    """[1,H,W] masks of the 16 x 8 pixel halves a wavefront of the blend kernels owns (rows 16 t + 8 w .. + 7 of tile column j)"""
    for y0 in range(0, H, 8):
        for x0 in range(0, W, 16):
            m = torch.zeros(1, H, W, device=dev)
            m[:, y0:y0 + 8, x0:x0 + 16] = 1.0
            yield m


def _a256(x):
    return (x + 255) & ~255


class Direct(NamedTuple):
    color: torch.Tensor
    depth: torch.Tensor
    alpha: torch.Tensor
    radii: torch.Tensor
    geometry: torch.Tensor        # the bytes of the geometry state that the projection writes
    backward: Callable            # (gc, gd, ga) -> [d_means3D, d_scales, d_rotations, d_opacities, d_shs, d_means2D, d_confidence]


def render_direct(lib, sc, dev, deg, family, raw=0, flags=0, filter3d=None, scale_modifier=1.0) -> Direct:
    """The scene `sc` (tests/raster_aa_ref.scene) through syn3r_raster_preprocess<family>, syn3r_raster_render and, on request,
    syn3r_raster_backward<family>.  `raw` (the "raw" family: always): the tensors are the parameters of raster_f3d_ref.raw_params;
    `raw` and `flags` go to the "ex" and "f3d" entries, `filter3d` (a device tensor or None = NULL) to the "f3d" ones.  Every state
    and output buffer starts from zeros, so two renders can be compared byte for byte.  `scale_modifier` goes to both passes; a scene
    whose "cf" is None (or missing) is rendered without a confidence (a null pointer; the backward's d_confidence buffer is still
    handed over and written)."""
    from syn3r_amd import _lib as L
    suffix, has_modes, has_filter = FAMILIES[family]
    raw = 1 if family == "raw" else raw
    assert has_modes or (flags == 0 and raw == (family == "raw")), "the old entries have no raw / flags arguments"
    assert has_filter or filter3d is None
    f = lambda t: t.float().to(dev).contiguous()
    N, H, W = sc["N"], sc["H"], sc["W"]
    p = F.raw_params(sc) if raw else sc
    m3, s, q, o, sh = f(sc["m"]), f(p["s"]), f(p["q"]), f(p["o"]), f(sc["sh"])
    cf = f(sc["cf"]) if sc.get("cf") is not None else None
    M = sh.shape[1]
    host = lambda t: L.host_f32(t.double().reshape(-1).tolist())
    view, proj, campos, bg = host(sc["view"].float()), host(sc["proj"].float()), host(sc["campos"].float()), host(sc["bg"].float())
    stream = L.stream_ptr(dev)
    tail = ((raw, flags) if has_modes else ()) + ((L.ptr(filter3d),) if has_filter else ()) + (stream,)
    u8 = lambda n: torch.zeros(max(int(n), 256), dtype=torch.uint8, device=dev)
    geom, image = u8(lib.syn3r_raster_geom_bytes(N)), u8(lib.syn3r_raster_image_bytes(H, W))
    radii = torch.zeros(N, dtype=torch.int32, device=dev)
    P = C.c_longlong(0)
    scene = (L.ptr(m3), L.ptr(s), L.ptr(q), L.ptr(o), L.ptr(sh), L.ptr(cf), float(scale_modifier), view, proj, campos, float(sc["tfx"]), float(sc["tfy"]), H, W)
    L.check(getattr(lib, "syn3r_raster_preprocess" + suffix)(N, deg, M, *scene, L.ptr(radii), L.ptr(geom), geom.numel(), C.byref(P), *tail),
            "preprocess" + suffix)
    P = int(P.value)
    binning = u8(lib.syn3r_raster_binning_bytes(P))
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
    color, depth, alpha = new(3, H, W), new(1, H, W), new(1, H, W)
    plist = C.c_void_p(0)
    L.check(lib.syn3r_raster_render(N, H, W, bg, L.ptr(radii), L.ptr(geom), geom.numel(), L.ptr(binning), binning.numel(), L.ptr(image),
                                    image.numel(), P, L.ptr(color), L.ptr(depth), L.ptr(alpha), C.byref(plist), stream), "render")
    # header, depths, means2D, cov3D, conic_opacity, rgb, clamped, tiles_touched, point_offsets, splats (csrc/raster_fwd.hip carve_geom)
    state = 256 + sum(_a256(N * b) for b in (4, 8, 24, 16, 12, 4, 4, 4, 48))
    geometry = geom[:state].clone()
    ws = u8(lib.syn3r_raster_backward_workspace_bytes(N))
    bwd = getattr(lib, "syn3r_raster_backward" + suffix)

    def backward(gc, gd, ga):
        d = [new(N, 3), new(N, 3), new(N, 4), new(N), new(N, M, 3), new(N, 3), new(N)]
        L.check(bwd(N, deg, M, P, *scene, bg, L.ptr(radii), L.ptr(geom), geom.numel(), plist.value, L.ptr(image), image.numel(),
                    L.ptr(gc), L.ptr(gd), L.ptr(ga), *[L.ptr(t) for t in d], L.ptr(ws), ws.numel(), *tail), "backward" + suffix)
        return d

    backward.keep = (m3, s, q, o, sh, cf, geom, image, binning, ws)      # the state lives as long as the closure
    backward.filter3d = filter3d
    return Direct(color, depth, alpha, radii, geometry, backward)
