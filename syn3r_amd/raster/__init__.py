"""Gaussian rasteriser on the HIP path, behind the Python interface FSGS's trainer binds
(`diff_gaussian_rasterization`-style `GaussianRasterizationSettings` / `GaussianRasterizer`,
returning colour, radii, depth and alpha, with a per-Gaussian `confidence`).

The reference reaches it through `gsTrainer.render_view(cam)` (model/diffusionGS.py:154,166)
and the trainer's loss.backward() (:139,1640).  Kernels: syn3r_raster_* in include/syn3r_hip.h.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from .. import _lib as L


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor      # world_view_transform (transposed w2c, as FSGS cameras store it)
    projmatrix: torch.Tensor      # full_proj_transform
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool = False
    debug: bool = False
    # The published rasteriser's switch (last field there too): anti-aliased splatting, the 2D Mip filter of Mip-Splatting.  The
    # 0.3 px^2 dilation stays and the blend opacity is multiplied by sqrt(max(det(cov2D) / det(cov2D + 0.3 I), 0.000025)), so a
    # splat keeps its energy whatever its size on screen (SYN3R_RASTER_ANTIALIAS in include/syn3r_hip.h; constants UNPINNED).
    # Off by default: FSGS' confidence fork is not known to have it.  Radii and tile lists do not depend on it.
    antialiasing: bool = False


_host_cache: dict = {}


def _host_floats(m: torch.Tensor):
    """Camera matrices / background live on the GPU in FSGS cameras; the ABI takes them by value.
    One device->host read per tensor OBJECT and version (the cache holds a weak reference to the tensor, so
    a recycled device address or an in-place update can never alias a stale copy)."""
    import weakref
    key = id(m)
    hit = _host_cache.get(key)
    if hit is not None and hit[0]() is m and hit[1] == m._version:
        return hit[2]
    if len(_host_cache) > 1024:
        for k in [k for k, v in _host_cache.items() if v[0]() is None]:
            del _host_cache[k]
    vals = L.host_f32(m.detach().to("cpu", torch.float32).reshape(-1).tolist())
    _host_cache[key] = (weakref.ref(m), m._version, vals)
    return vals


# ---- pair-count mode ------------------------------------------------------------------------------------
# "sync"  (default): read the exact number of (Gaussian, tile) pairs back after the projection stage, as the
#                    published implementation does, and size the binning buffer exactly.
# "async" (opt-in, training loops): size the binning buffer from the previous calls of the same shape (x2),
#                    let the kernels read the live count on the device, and check the overflow flag of call k
#                    at call k+1 (or at `flush_pair_checks()`): a call that overflowed raises then — its image
#                    was built from a truncated pair list.  Removes the one host<->device round trip per render.
_HEADROOM = 2.0          # async capacity = 2 x the largest pair count seen for the shape (24 B per pair: ~125 MB at 2.6 M pairs)
_pair_mode = "sync"
_capacity: dict = {}
_pending: dict = {}


def set_pair_count_mode(mode: str) -> None:
    global _pair_mode
    if mode not in ("sync", "async"):
        raise ValueError("pair-count mode must be 'sync' or 'async'")
    _pair_mode = mode


def get_pair_count_mode() -> str:
    return _pair_mode


def _check_pending(key, wait: bool) -> int:
    """Examine finished renders of this shape (all of them if `wait`), oldest first; never blocks the host unless
    asked to or more than 8 renders are unchecked.  Returns how many of the examined renders had outgrown their binning
    buffer (their images were built from a truncated pair list); the capacity of the shape is raised on the way."""
    queue = _pending.get(key)
    truncated = 0
    while queue:
        evt, host, cap = queue[0]
        if not (wait or len(queue) > 8 or evt.query()):
            break
        evt.synchronize()
        queue.pop(0)
        P, overflow = int(host[0]), int(host[1])
        _capacity[key] = max(_capacity.get(key, 0), int(P * _HEADROOM) + 4096)
        if overflow or P > cap:
            truncated += 1
    if queue is not None and not queue:
        del _pending[key]
    return truncated


def _overflow_error(n: int) -> "L.Syn3rError":
    return L.Syn3rError(f"rasteriser (async pair-count mode): {n} previous render(s) needed more (Gaussian, tile) pairs than "
                        "the binning buffer held; those images are invalid - capacity has been raised, render again")


def flush_pair_checks() -> int:
    """Verify the overflow flag of EVERY render still unchecked, for every shape (call at the end of a training loop).
    All queues are drained before anything is raised; the error carries the total in `.truncated`."""
    total = 0
    for key in list(_pending):
        total += _check_pending(key, wait=True)
    if total:
        err = _overflow_error(total)
        err.truncated = total
        raise err
    return 0


def carry_capacity(old_key, new_key, scale: float) -> None:
    """A change of the Gaussian count (densification) changes the capacity key (device, N, H, W).  Start the new shape
    from the old one's capacity scaled by N_new / N_old instead of from the next single view's count, and forget the
    old key (its renders have been checked by then: call after `flush_pair_checks`)."""
    cap = _capacity.pop(old_key, None)
    _pending.pop(old_key, None)
    if cap is not None:
        _capacity[new_key] = max(_capacity.get(new_key, 0), int(cap * max(scale, 1.0)) + 4096)


def capacity_key(dev: torch.device, N: int, H: int, W: int):
    return (dev.index, int(N), int(H), int(W))


def _flags(s: GaussianRasterizationSettings) -> int:
    """the `flags` of syn3r_raster_preprocess_f3d / syn3r_raster_backward_f3d (and _abs, _cam) for these settings"""
    return L.RASTER_ANTIALIAS if s.antialiasing else 0


class RasterState:
    """What `rasterize_forward` leaves for `rasterize_backward`: the (detached, contiguous fp32) inputs, the device state of the two
    forward stages and the host-side constants.  `scene` is the argument prefix of the projection entry (N, sh_degree, sh_coeffs (`M`),
    the six input tensors by address, scale_modifier, the camera by value, H, W) and `bwd_scene` the same with `P` after `M`, the
    prefix of the backward entries: both built once, so the backward cannot describe another scene than the forward did;
    `addresses` are those of the five Gaussian tensors.  `tensors` holds the ten device tensors in the order of the names below,
    which read it.  A plain object: the autograd Function stores `tensors` through `save_for_backward`, a caller that drives the two
    passes itself (`GSTrainer._explicit_step`) just keeps it."""
    __slots__ = ("settings", "N", "M", "H", "W", "scene", "bwd_scene", "addresses", "bg", "P", "plist", "has_conf", "opacity_shape",
                 "raw_params", "tensors", "filter_3D")
    means3D, scales, rotations, opacities, shs, confidence, radii, geom, binning, image = (
        property(lambda st, i=i: st.tensors[i]) for i in range(10))


def rasterize_forward(means3D, shs, opacities, scales, rotations, confidence, settings: GaussianRasterizationSettings,
                      raw_params: bool = False, filter_3D: Optional[torch.Tensor] = None):
    """Both forward stages (`syn3r_raster_preprocess_f3d`, `syn3r_raster_render`); returns (color, radii, depth, alpha, state).
    `raw_params`: `scales`, `rotations`, `opacities` are the trainer's PARAMETERS (log-scales, unnormalised quaternions, logits);
    the published activations run inside the projection kernel and `rasterize_backward` returns the gradients of the parameters
    (`syn3r_raster_backward_f3d` with raw = 1).  `settings.antialiasing` goes to both passes as SYN3R_RASTER_ANTIALIAS: the state
    keeps the settings, so `rasterize_backward` cannot be given another mode than the forward.
    `filter_3D` ([N] fp32, default None = the unfiltered render, bit for bit): Mip-Splatting's 3D smoothing filter
    (`train_ops.compute_filter_3D`), applied to the scales and the opacity inside the projection kernel; the state remembers it for
    `rasterize_backward`.  It is data: no gradient flows into it."""
    s = settings
    dev = L.require_gpu(means3D, shs, opacities, scales, rotations)
    lib = L.load()
    N = means3D.shape[0]
    H, W = int(s.image_height), int(s.image_width)
    if N == 0:
        raise ValueError("rasteriser needs at least one Gaussian")
    M = shs.shape[1]
    f32 = lambda t: t.detach().to(torch.float32).contiguous()
    m3, sh, op, sc, ro = f32(means3D), f32(shs), f32(opacities).reshape(-1), f32(scales), f32(rotations)
    cf = f32(confidence).reshape(-1) if confidence is not None else None
    f3 = None
    if filter_3D is not None:
        L.require_gpu(means3D, filter_3D)
        f3 = f32(filter_3D).reshape(-1)
        if f3.shape != (N,):
            raise ValueError(f"rasteriser: filter_3D must hold one value per Gaussian ({N}), got {tuple(filter_3D.shape)}")
    if m3.shape != (N, 3) or sc.shape != (N, 3) or ro.shape != (N, 4) or op.shape != (N,) or sh.shape != (N, M, 3):
        raise ValueError("rasteriser: inconsistent Gaussian tensor shapes")
    bg = _host_floats(s.bg)
    dims, addresses = (N, int(s.sh_degree), M), (L.ptr(m3), L.ptr(sc), L.ptr(ro), L.ptr(op), L.ptr(sh))
    rest = (*addresses, L.ptr(cf), float(s.scale_modifier), _host_floats(s.viewmatrix), _host_floats(s.projmatrix),
            _host_floats(s.campos), float(s.tanfovx), float(s.tanfovy), H, W)
    scene = (*dims, *rest)
    stream = L.stream_ptr(dev)

    geom = torch.empty(lib.syn3r_raster_geom_bytes(N), dtype=torch.uint8, device=dev)
    image = torch.empty(lib.syn3r_raster_image_bytes(H, W), dtype=torch.uint8, device=dev)
    radii = torch.empty(N, dtype=torch.int32, device=dev)
    key = (dev.index, N, H, W)
    use_async = _pair_mode == "async" and not s.debug
    if use_async:
        n_trunc = _check_pending(key, wait=False)
        if n_trunc:
            err = _overflow_error(n_trunc)
            err.truncated = n_trunc
            raise err
    use_async = use_async and key in _capacity
    P = C.c_longlong(0)
    rc = lib.syn3r_raster_preprocess_f3d(*scene, L.ptr(radii), L.ptr(geom), geom.numel(), None if use_async else C.byref(P),
                                         int(bool(raw_params)), _flags(s), L.ptr(f3), stream)
    L.check(rc, "syn3r_raster_preprocess_f3d")
    if use_async:
        P = _capacity[key]                          # capacity; the kernels read the live count on the device
    else:
        P = int(P.value)
        _capacity[key] = max(_capacity.get(key, 0), int(P * _HEADROOM) + 4096)
    binning = torch.empty(lib.syn3r_raster_binning_bytes(P), dtype=torch.uint8, device=dev)
    color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    depth = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    alpha = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    plist = C.c_void_p(0)
    rc = lib.syn3r_raster_render(N, H, W, bg, L.ptr(radii), L.ptr(geom), geom.numel(), L.ptr(binning),
                                 binning.numel(), L.ptr(image), image.numel(), P, L.ptr(color), L.ptr(depth),
                                 L.ptr(alpha), C.byref(plist), stream)
    L.check(rc, "syn3r_raster_render")
    if use_async:
        host = torch.empty(2, dtype=torch.int32, pin_memory=True)
        host.copy_(geom[:8].view(torch.int32), non_blocking=True)
        evt = torch.cuda.Event()
        evt.record(torch.cuda.current_stream(dev))
        _pending.setdefault(key, []).append((evt, host, P))
    if s.debug:   # expose the binning / image state (tile ranges, sorted list) to the parity tests
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        a256 = lambda x: (x + 255) & ~255
        off = plist.value - binning.data_ptr() if P > 0 else 0
        _Rasterize.debug_state = dict(
            num_rendered=P,
            point_list=binning[off:off + 4 * P].view(torch.int32).clone(),
            ranges=image[:tiles * 8].view(torch.int32).reshape(tiles, 2).clone(),
            n_contrib=image[a256(tiles * 8):a256(tiles * 8) + 4 * H * W].view(torch.int32).reshape(H, W).clone(),
            depths=geom[256:256 + 4 * N].view(torch.float32).clone(),
        )
    st = RasterState()
    st.settings, st.scene, st.bwd_scene, st.addresses, st.bg, st.P, st.plist = s, scene, (*dims, P, *rest), addresses, bg, P, plist.value
    st.N, st.M, st.H, st.W = N, M, H, W
    st.has_conf, st.opacity_shape, st.raw_params = cf is not None, opacities.shape, bool(raw_params)
    st.filter_3D = f3
    st.tensors = (m3, sc, ro, op, sh, cf if cf is not None else torch.empty(0, device=dev), radii, geom, binning, image)
    return color, radii, depth, alpha, st


def _out_buffer(name: str, t: torch.Tensor, shape: tuple, dev: torch.device) -> int:
    """the address of an output buffer of `rasterize_backward`: a contiguous fp32 tensor of `shape` on the state's device"""
    if t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"rasterize_backward: {name} must be a contiguous {list(shape)} float32 tensor on {dev}")
    return L.ptr(t)


def rasterize_backward(st: RasterState, g_color, g_depth=None, g_alpha=None, abs_grad_out: Optional[torch.Tensor] = None,
                       camera_grad_out: Optional[torch.Tensor] = None, camera_grad_accumulate: bool = False):
    """Backward of both stages (`syn3r_raster_backward_f3d`, in the forward's mode and with the forward's `filter_3D`): (d_means3D,
    d_means2D, d_shs, d_opacities, d_scales, d_rotations, d_confidence or None) - with `raw_params` the gradients of the log-scales /
    raw quaternions / logits.  The entry is chosen HERE and nowhere else, from the two optional output buffers.
    `abs_grad_out` (default None: that entry): a contiguous [N,2] fp32 tensor on the state's device that `syn3r_raster_backward_abs`
    fills with AbsGS' absolute screen-space gradient, per Gaussian the sum over its pixels of the component-wise |d loss / d projected
    mean| in the units of d_means2D[:, :2] (zeros for culled Gaussians).  The returned tuple is the same either way.
    `camera_grad_out` (EXTENSION, default None: one of the two entries above): a contiguous [35] fp32 tensor on the state's device that
    `syn3r_raster_backward_cam` fills with the gradient with respect to the camera - d loss / d viewmatrix [16], / d projmatrix [16],
    / d campos [3], each in its tensor's storage order, the three taken as INDEPENDENT inputs (`syn3r_amd.gs.pose.tangent_from_raw`
    turns them into the gradient of a pose); with `camera_grad_accumulate` it is ADDED to what the tensor holds.  Same tuple again."""
    if (L.ptr(st.means3D), L.ptr(st.scales), L.ptr(st.rotations), L.ptr(st.opacities), L.ptr(st.shs)) != st.addresses:
        raise L.Syn3rError("rasterize_backward: the state's tensors are not the ones rasterize_forward stored")
    lib = L.load()
    radii, geom, image = st.radii, st.geom, st.image
    dev, N, M = radii.device, st.N, st.M
    # the entry and what it takes after the common arguments; with neither buffer the call is the one made before they existed
    entry, ws_bytes, extra = "syn3r_raster_backward_f3d", lib.syn3r_raster_backward_workspace_bytes, ()
    if abs_grad_out is not None:
        entry, extra = "syn3r_raster_backward_abs", (_out_buffer("abs_grad_out", abs_grad_out, (N, 2), dev),)
    if camera_grad_out is not None:
        entry, ws_bytes = "syn3r_raster_backward_cam", lib.syn3r_raster_backward_cam_workspace_bytes
        extra = (L.ptr(abs_grad_out), _out_buffer("camera_grad_out", camera_grad_out, (L.CAMERA_GRAD,), dev),
                 int(bool(camera_grad_accumulate)))
    gc = g_color.detach().to(torch.float32).contiguous() if g_color is not None else torch.zeros((3, st.H, st.W), device=dev)
    gd = g_depth.detach().to(torch.float32).contiguous() if g_depth is not None else None
    ga = g_alpha.detach().to(torch.float32).contiguous() if g_alpha is not None else None
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    d_m3, d_sc, d_ro, d_op, d_sh, d_m2 = new(N, 3), new(N, 3), new(N, 4), new(N), new(N, M, 3), new(N, 3)
    d_cf = new(N) if st.has_conf else None
    ws = L.workspace(dev, ws_bytes(N), "raster_bwd")
    rc = getattr(lib, entry)(*st.bwd_scene, st.bg, L.ptr(radii), L.ptr(geom), geom.numel(), st.plist, L.ptr(image), image.numel(),
                             L.ptr(gc), L.ptr(gd), L.ptr(ga), L.ptr(d_m3), L.ptr(d_sc), L.ptr(d_ro), L.ptr(d_op), L.ptr(d_sh),
                             L.ptr(d_m2), L.ptr(d_cf), L.ptr(ws), ws.numel(), int(st.raw_params), _flags(st.settings),
                             L.ptr(st.filter_3D), *extra, L.stream_ptr(dev))
    L.check(rc, entry)
    return d_m3, d_m2, d_sh, d_op.reshape(st.opacity_shape), d_sc, d_ro, d_cf


class _Rasterize(torch.autograd.Function):
    """autograd around `rasterize_forward` / `rasterize_backward` (activated tensors in, as the published rasteriser takes them)."""
    debug_state = None

    @staticmethod
    def forward(ctx, means3D, means2D, shs, opacities, scales, rotations, confidence, settings, filter_3D, means2D_abs, camera_grad,
                camera_grad_accumulate):
        color, radii, depth, alpha, st = rasterize_forward(means3D, shs, opacities, scales, rotations, confidence, settings,
                                                           filter_3D=filter_3D)
        ctx.means2D_abs = means2D_abs        # a buffer the backward fills (`GaussianRasterizer.forward`), not an input of the render
        ctx.camera_grad, ctx.camera_grad_accumulate = camera_grad, bool(camera_grad_accumulate)      # likewise
        ctx.save_for_backward(*st.tensors)
        st.tensors = None
        ctx.state = st
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)     # unused outputs (depth / alpha) arrive as None, not as zero tensors
        return color, radii, depth, alpha

    @staticmethod
    def backward(ctx, g_color, g_radii, g_depth, g_alpha):
        L.join_active_trace()        # autograd thread: record into the caller's kernel_trace session, if one is open
        st = ctx.state
        st.tensors = ctx.saved_tensors
        try:
            d_m3, d_m2, d_sh, d_op, d_sc, d_ro, d_cf = rasterize_backward(
                st, g_color, g_depth, g_alpha, abs_grad_out=ctx.means2D_abs, camera_grad_out=ctx.camera_grad,
                camera_grad_accumulate=ctx.camera_grad_accumulate)
        finally:
            st.tensors = None
        # one per argument of `forward`: settings, filter_3D, means2D_abs, camera_grad and camera_grad_accumulate have no gradient
        return d_m3, d_m2, d_sh, d_op, d_sc, d_ro, d_cf, None, None, None, None, None


class GaussianRasterizer(torch.nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, confidence: Optional[torch.Tensor] = None, filter_3D: Optional[torch.Tensor] = None,
                means2D_abs: Optional[torch.Tensor] = None, camera_grad: Optional[torch.Tensor] = None,
                camera_grad_accumulate: bool = False):
        """`camera_grad` (EXTENSION, default None): a [35] fp32 buffer on the Gaussians' device that the autograd backward of this
        render fills with (or, with `camera_grad_accumulate`, adds to it) the gradient with respect to the camera
        (`rasterize_backward(camera_grad_out=)`).  Handled like `means2D_abs`: data, not an input of the render.
        `means2D_abs` (default None): an [N,2] fp32 buffer on the Gaussians' device that the autograd backward of this render
        FILLS with AbsGS' absolute screen-space gradient (`rasterize_backward(abs_grad_out=)`).  It is data: no gradient flows into
        it or out of it, and the render does not read it."""
        if (shs is None) == (colors_precomp is None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if colors_precomp is not None or cov3D_precomp is not None:
            raise NotImplementedError("precomputed colours / covariances are not used by the SYN3R hot path")
        if scales is None or rotations is None:
            raise Exception("Please provide scales and rotations")
        if filter_3D is not None:
            filter_3D = filter_3D.detach()       # data (Mip-Splatting's 3D smoothing filter, `rasterize_forward`): no gradient
        if means2D_abs is not None and means2D_abs.requires_grad:
            raise ValueError("GaussianRasterizer: means2D_abs is a buffer the backward fills, not a tensor that requires grad")
        if camera_grad is not None and camera_grad.requires_grad:
            raise ValueError("GaussianRasterizer: camera_grad is a buffer the backward fills, not a tensor that requires grad")
        return _Rasterize.apply(means3D, means2D, shs, opacities, scales, rotations, confidence, self.raster_settings, filter_3D,
                                means2D_abs, camera_grad, bool(camera_grad_accumulate))


def sort_pairs(keys: torch.Tensor, vals: torch.Tensor, nbits: int = 64):
    """Stable radix sort of (int64/uint64-bit-pattern key, int32 value) pairs on the GPU."""
    dev = L.require_gpu(keys, vals)
    lib = L.load()
    n = keys.numel()
    k = keys.contiguous().clone()
    v = vals.contiguous().clone()
    kt, vt = torch.empty_like(k), torch.empty_like(v)
    ws = L.workspace(dev, lib.syn3r_sort_pairs_workspace_bytes(n), "sort")
    flag = C.c_int(0)
    rc = lib.syn3r_sort_pairs(L.ptr(k), L.ptr(v), L.ptr(kt), L.ptr(vt), n, nbits, L.ptr(ws), ws.numel(), C.byref(flag),
                              L.stream_ptr(dev))
    L.check(rc, "syn3r_sort_pairs")
    return (kt, vt) if flag.value else (k, v)
