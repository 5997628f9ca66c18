"""The patch-wise depth-correlation term (csrc/depth_loss.hip, train_ops.depth_correlation_local_loss[_step]) against its float64
restatement (tests/depth_local_ref.py): every mapping of the statistics pass, planted patches, independence of the patches,
poisoned buffers, repeatability, and the trainer with the term on.

Bars (the global term's, tests/test_depth_loss_gpu.py, per patch): loss 1e-5 relative, parts[1] 1e-6, per-patch gradient error
1e-5 of the patch's largest reference entry, the chosen branch equal to the reference's wherever the reference's |L_A - L_B| exceeds
1e-9, and at most 1 % of the patches left out for that reason.  The gradient of a left-out patch that took the other branch is not
compared: it is the gradient of another, equally good, branch."""
import math

import numpy as np
import pytest
import torch

from oracle import raster_oracle as RO
from tests import depth_local_ref as R
from tests.depth_terms import prior as _prior, same as _same, scene as _scene, spy_rasterize_backward, step_bits as _step_bits
from tests.poison import PATTERNS, poisoned
from tests.test_depth_loss_gpu import make_case as global_case

pytestmark = pytest.mark.gpu

# (H, W, P, oy, ox): partial borders, odd patch sizes, both sides of the wave-per-strip / block-per-strip switch (P = 16 | 17) and of
# the 4-wave / 16-wave block switch (P = 64 | 65: a patch wider than a wave), the largest patch, several strips per patch row, and
# (BIG) a grid large enough for more than one wave of blocks
SHAPES = [(37, 53, 8, 5, 3), (37, 53, 2, 1, 1), (37, 53, 3, 0, 2), (72, 104, 16, 7, 9), (72, 104, 17, 0, 0), (130, 150, 64, 2, 22),
          (300, 520, 256, 3, 5), (131, 150, 65, 0, 1)]
BIG = (1080, 1920, 32, 11, 13)
KINDS = ["random", "cancel", "inv"]
GAP = 1e-9


def make_case(kind, H, W, seed):
    """The global term's fields (tests/test_depth_loss_gpu.py::make_case); the cancelling one - depths at 50 with a spread of 1e-3,
    where sum(x^2) - n mean^2 would cancel - with a prior spread wide enough (100 +- 40) for 1 / (p + 200) to bend: under the global
    test's prior (0.02 +- 1e-4) the two transforms are one line to 1e-9 and the reference itself cannot tell the branches apart."""
    if kind != "cancel":
        return global_case(kind, H, W, seed)
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(H, W, generator=g)
    d = 50.0 + 1e-3 * z
    p = 100.0 + 40.0 * (0.7 * z + 0.7 * torch.randn(H, W, generator=g))
    return d.float()[None].contiguous(), p.float().clamp_min(-150.0).contiguous()


def _ops():
    from syn3r_amd.gs import train_ops
    return train_ops.depth_correlation_local_loss, train_ops.depth_correlation_local_loss_step, train_ops.depth_correlation_local_records


def _per_patch_max(x, idx, K):
    """max over each patch of x [H,W] (idx: the patch of a pixel, -1 none) -> [K]"""
    inside = idx >= 0
    return torch.zeros(K, dtype=x.dtype).scatter_reduce(0, idx[inside], x[inside], "amax", include_self=True)


def _against_ref(d, p, geom, w, gpu, mode="min"):
    """One step on (d [1,H,W], p [H,W]) held to every bar; -> the measured figures"""
    _, step, records = _ops()
    H, W, P, oy, ox = geom
    ref = R.ref_local(d, p, w, P, (oy, ox), mode=mode)
    K = ref["K"]
    loss, grad, parts = step(d.to(gpu), p.to(gpu), w, P, (oy, ox), mode=mode, return_parts=True)
    rec = records(d.to(gpu), p.to(gpu), P, (oy, ox), mode=mode).cpu()
    parts, grad = parts.cpu(), grad.cpu()
    assert loss.shape == () and loss.is_cuda and grad.shape == d.shape and rec.shape == (ref["lk"].shape + (8,))
    assert torch.isfinite(parts).all() and torch.isfinite(grad).all() and torch.isfinite(rec).all()
    lerr = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
    rerr = abs(float(parts[1]) - ref["parts"][1])
    # the branch of every patch, wherever the reference can tell
    decided = ref["gap"] > GAP if mode == "min" else torch.ones_like(ref["gap"], dtype=torch.bool)
    left_out = 1.0 - float(decided.double().mean())
    same = rec[..., 6] == ref["branch"]
    assert bool(same[decided].all()), f"{int((~same[decided]).sum())} decided patches took the other branch"
    assert torch.equal(rec[..., 7], ref["flat"])
    # the gradient per patch, and exact zeros in no full patch
    idx = R.patch_of(H, W, P, oy, ox)
    assert not grad[0][idx < 0].any()
    err = _per_patch_max((grad[0].double() - ref["grad"]).abs(), idx, K) / ref["gmax"].reshape(-1).clamp_min(1e-300)
    err = torch.where(ref["flat"].reshape(-1) > 0, torch.zeros_like(err), err)[same.reshape(-1)]
    assert not grad[0][(idx >= 0) & (ref["flat"].reshape(-1)[idx.clamp_min(0)] > 0)].any()
    gerr = float(err.max()) if err.numel() else 0.0
    fig = dict(loss_rel=lerr, r_abs=rerr, grad_rel=gerr, left_out=left_out, share_b=float(parts[2]), share_flat=float(parts[3]), K=K)
    print(f"depth_local {geom} mode={mode}: {fig}")
    assert lerr <= 1e-5, (float(loss), ref["loss"])
    assert rerr <= 1e-6, (float(parts[1]), ref["parts"][1])
    assert gerr <= 1e-5, gerr
    assert left_out <= 0.01, left_out
    assert abs(float(parts[2]) - float(rec[..., 6].mean())) <= 1e-6 and abs(float(parts[3]) - ref["parts"][3]) <= 1e-6
    return fig, ref


@pytest.mark.parametrize("geom", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_op_matches_float64_restatement(kind, geom, gpu, measurements):
    H, W = geom[:2]
    d, p = make_case(kind, H, W, seed=H + 7 * KINDS.index(kind) + geom[2])
    fig, ref = _against_ref(d, p, geom, 0.3, gpu)
    measurements("depth_local_op", kind=kind, geom=list(geom), **fig)
    if kind == "random" and geom[2] != 256:       # both branches are exercised, and no patch is flat
        assert ref["parts"][3] == 0.0 and 0.0 < ref["parts"][2] < 1.0
    if kind == "inv" and geom[2] >= 8:
        assert ref["parts"][2] > 0.5


def test_large_grid_once(gpu, measurements):
    H, W = BIG[:2]
    d, p = make_case("random", H, W, seed=5)
    fig, _ = _against_ref(d, p, BIG, 0.3, gpu)
    measurements("depth_local_op", kind="random", geom=list(BIG), **fig)


@pytest.mark.parametrize("mode", ["A", "B"])
def test_single_branch_modes(mode, gpu):
    d, p = make_case("random", 72, 104, seed=9)
    _against_ref(d, p, (72, 104, 16, 7, 9), 0.3, gpu, mode=mode)
    _against_ref(d, p, (72, 104, 17, 0, 0), 0.3, gpu, mode=mode)


# ---------------------------------------------------------------- planted cases
def test_constant_patch_counts_one_and_has_no_gradient(gpu):
    _, step, records = _ops()
    H, W, P, oy, ox = 72, 104, 16, 7, 9
    d, p = make_case("random", H, W, seed=2)
    d[0, oy + P:oy + 2 * P, ox + 2 * P:ox + 3 * P] = 7.0         # patch (1, 2)
    ref = R.ref_local(d, p, 1.0, P, (oy, ox))
    K = ref["K"]
    assert ref["flat"].sum() == 1 and ref["flat"][1, 2] == 1 and ref["lk"][1, 2] == 1.0
    loss, grad, parts = step(d.to(gpu), p.to(gpu), 1.0, P, (oy, ox), return_parts=True)
    rec = records(d.to(gpu), p.to(gpu), P, (oy, ox)).cpu()
    assert float(rec[1, 2, 4]) == 1.0 and float(rec[1, 2, 5]) == 0.0 and float(rec[1, 2, 7]) == 1.0 and rec[..., 7].sum() == 1
    assert not grad[0, oy + P:oy + 2 * P, ox + 2 * P:ox + 3 * P].any()
    assert float(parts[3]) == float(np.float32(1.0 / K))
    assert abs(float(loss) - ref["loss"]) <= 1e-5 * ref["loss"]
    assert torch.isfinite(grad).all()
    idx = R.patch_of(H, W, P, oy, ox)
    others = (idx >= 0) & (idx != 1 * ref["lk"].shape[1] + 2)
    assert float((grad[0].cpu().double() - ref["grad"]).abs()[others].max()) <= 1e-5 * float(ref["gmax"].max())


def test_planted_inverse_patch_takes_b_among_a_neighbours(gpu):
    _, _, records = _ops()
    H, W, P, oy, ox = 72, 104, 16, 3, 4
    g = torch.Generator().manual_seed(4)
    p = torch.rand(H, W, generator=g) * 5000.0
    d = 30.0 - 0.004 * p + 0.05 * torch.randn(H, W, generator=g)          # disparity-like: linear in -p
    ys, xs = slice(oy + 2 * P, oy + 3 * P), slice(ox + 3 * P, ox + 4 * P)      # patch (2, 3)
    d[ys, xs] = (1.0 / (p[ys, xs] + 200.0)) * (1.0 + 0.01 * torch.randn(P, P, generator=g))
    ref = R.ref_local(d, p, 1.0, P, (oy, ox))
    want = torch.zeros_like(ref["branch"])
    want[2, 3] = 1.0
    assert torch.equal(ref["branch"], want) and float(ref["gap"].min()) > 1e-3
    rec = records(d[None].float().to(gpu), p.to(gpu), P, (oy, ox)).cpu()
    assert torch.equal(rec[..., 6], want)


@pytest.mark.parametrize("side", [48, 96])
def test_one_patch_over_the_image_is_the_global_term(side, gpu):
    from syn3r_amd.gs.train_ops import depth_correlation_loss_step
    _, step, _ = _ops()
    d, p = make_case("random", side, side, seed=side)
    d, p = d.to(gpu), p.to(gpu)
    lg, gg = depth_correlation_loss_step(d, p, 0.3)
    ll, gl = step(d, p, 0.3, side)
    assert abs(float(ll) - float(lg)) <= 1e-6 * abs(float(lg))
    assert float((gl - gg).abs().max()) <= 1e-5 * float(gg.abs().max())


# ---------------------------------------------------------------- independence and invariance
def test_patches_are_independent(gpu):
    _, step, _ = _ops()
    for H, W, P, oy, ox in ((72, 104, 16, 7, 9), (72, 104, 17, 0, 0), (130, 150, 64, 2, 22)):
        d, p = make_case("random", H, W, seed=6)
        _, g1 = step(d.to(gpu), p.to(gpu), 0.3, P, (oy, ox))
        d2 = d.clone()
        ys, xs = slice(oy + P, oy + 2 * P), slice(ox, ox + P)                   # patch (1, 0)
        d2[0, ys, xs] += torch.rand(P, P, generator=torch.Generator().manual_seed(1))
        _, g2 = step(d2.to(gpu), p.to(gpu), 0.3, P, (oy, ox))
        mask = torch.ones(H, W, dtype=torch.bool)
        mask[ys, xs] = False
        assert torch.equal(g1[0].cpu()[mask], g2[0].cpu()[mask])
        assert not torch.equal(g1[0].cpu()[~mask], g2[0].cpu()[~mask])


def test_per_patch_affine_maps_keep_the_loss(gpu, measurements):
    """d -> 2^a_k d + b_k per patch (a_k, b_k small integers) keeps every patch's Pearson coefficients, hence the loss; the global
    term sees a scrambled image."""
    from syn3r_amd.gs.train_ops import depth_correlation_loss_step
    _, step, _ = _ops()
    H, W, P, oy, ox = 72, 104, 16, 7, 9
    d, p = make_case("random", H, W, seed=12)
    PY, PX = R.grid(H, W, P, oy, ox)
    g = torch.Generator().manual_seed(3)
    a = torch.randint(-2, 3, (PY, PX), generator=g)
    b = torch.randint(-3, 4, (PY, PX), generator=g)
    d2 = d.clone()
    for i in range(PY):
        for j in range(PX):
            ys, xs = slice(oy + i * P, oy + (i + 1) * P), slice(ox + j * P, ox + (j + 1) * P)
            d2[0, ys, xs] = d[0, ys, xs] * float(2.0 ** int(a[i, j])) + float(b[i, j])
    l1, _ = step(d.to(gpu), p.to(gpu), 1.0, P, (oy, ox))
    l2, _ = step(d2.to(gpu), p.to(gpu), 1.0, P, (oy, ox))
    g1, _ = depth_correlation_loss_step(d.to(gpu), p.to(gpu), 1.0)
    g2, _ = depth_correlation_loss_step(d2.to(gpu), p.to(gpu), 1.0)
    measurements("depth_local_invariance", local=[float(l1), float(l2)], glob=[float(g1), float(g2)])
    assert abs(float(l2) - float(l1)) <= 1e-5 * abs(float(l1)), (float(l1), float(l2))
    assert abs(float(g2) - float(g1)) > 0.05, (float(g1), float(g2))


# ---------------------------------------------------------------- poisoned output, accumulate
def test_poisoned_buffers_and_accumulate(gpu, monkeypatch):
    _, step, _ = _ops()
    for H, W, P, oy, ox in ((37, 53, 8, 5, 3), (72, 104, 17, 0, 0), (130, 150, 64, 2, 22)):
        d, p = make_case("random", H, W, seed=8)
        d, p = d.to(gpu), p.to(gpu)
        inside = (R.patch_of(H, W, P, oy, ox) >= 0).to(gpu)
        assert bool((~inside).any())
        outs = []
        for byte in PATTERNS:
            with poisoned(monkeypatch, byte):
                loss, grad, parts = step(d, p, 0.3, P, (oy, ox), return_parts=True)
                torch.cuda.synchronize()
                assert not grad[0][~inside].view(torch.int32).any()              # exactly +0
                assert torch.isfinite(grad).all() and torch.isfinite(parts).all()
                outs.append((loss.clone(), grad, parts))
                # a given buffer is added to inside the patches and keeps its bits elsewhere
                buf = torch.empty(1, H, W, device=gpu)                           # (the pattern)
                buf[0][inside] = torch.randn(int(inside.sum()), generator=torch.Generator().manual_seed(byte)).to(gpu)
                prev = buf.clone()
                loss_a, grad_a = step(d, p, 0.3, P, (oy, ox), grad_out=buf)
                torch.cuda.synchronize()
                assert grad_a.data_ptr() == buf.data_ptr() and torch.equal(loss_a, loss)
                assert torch.equal(buf[0][~inside].view(torch.int32), prev[0][~inside].view(torch.int32))
                want = prev[0][inside].double() + grad[0][inside].double()
                tol = 1.2e-7 * (prev[0][inside].abs() + grad[0][inside].abs()).double()
                assert bool(((buf[0][inside].double() - want).abs() <= tol).all())
        for o in outs[1:]:
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(outs[0], o))


# ---------------------------------------------------------------- repeatability
@pytest.mark.parametrize("geom", [(72, 104, 16, 7, 9), (72, 104, 17, 0, 0), (300, 520, 256, 3, 5)])
def test_bitwise_repeatable_and_grad_loss_scaling(geom, gpu):
    local, step, _ = _ops()
    H, W, P, oy, ox = geom
    d, p = make_case("random", H, W, seed=11)
    d, p = d.to(gpu), p.to(gpu)
    l1, g1 = step(d, p, 0.05, P, (oy, ox))
    l2, g2 = step(d, p, 0.05, P, (oy, ox))
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    # value-only entry = step entry; autograd backward = step gradient, bit for bit
    x = d.clone().requires_grad_(True)
    la, pa = local(x, p, 0.05, P, (oy, ox), return_parts=True)
    la.backward()
    _, _, ps = step(d, p, 0.05, P, (oy, ox), return_parts=True)
    assert torch.equal(la.detach(), l1) and torch.equal(x.grad, g1) and torch.equal(pa, ps)
    # grad_loss: a power of two scales exactly; any other value equals autograd's upstream scalar
    _, g4 = step(d, p, 0.05, P, (oy, ox), grad_loss=torch.tensor(2.0, device=gpu))
    assert torch.equal(g4, 2.0 * g1)
    x.grad = None
    (local(x, p, 0.05, P, (oy, ox)) * 0.37).backward()
    _, g37 = step(d, p, 0.05, P, (oy, ox), grad_loss=torch.tensor(0.37, device=gpu))
    assert torch.equal(x.grad, g37)
    assert float((g37.double() - 0.37 * g1.double()).abs().max()) <= 1e-6 * float(g1.abs().max())


@pytest.mark.parametrize("geom", [(37, 53, 8, 5, 3), (72, 104, 17, 0, 0), (130, 150, 64, 2, 22)])
def test_misaligned_inputs(geom, gpu):
    """d offset by 1 float and p by 3 from a 16-byte boundary: the same results within the bars"""
    H, W = geom[:2]
    d, p = make_case("random", H, W, seed=3)
    buf_d = torch.zeros(H * W + 1, device=gpu)
    buf_p = torch.zeros(H * W + 3, device=gpu)
    buf_d[1:] = d.reshape(-1).to(gpu)
    buf_p[3:] = p.reshape(-1).to(gpu)
    dm, pm = buf_d[1:].view(1, H, W), buf_p[3:].view(H, W)
    assert dm.data_ptr() % 16 and pm.data_ptr() % 16
    _, step, _ = _ops()
    P, o = geom[2], geom[3:]
    la, ga = step(d.to(gpu), p.to(gpu), 0.3, P, o)
    lm, gm = step(dm, pm, 0.3, P, o)
    assert torch.equal(la, lm) and torch.equal(ga, gm)        # the loads are 4-byte either way: the same arithmetic
    _against_ref(dm.cpu(), pm.cpu(), geom, 0.3, gpu)


def test_op_rejects_bad_arguments(gpu):
    from syn3r_amd import _lib
    local, step, _ = _ops()
    d = torch.rand(1, 16, 16, device=gpu)
    for bad in (torch.rand(16, 17, device=gpu), torch.rand(2, 16, 16, device=gpu), torch.rand(256, device=gpu),
                torch.rand(16, 16, device=gpu).half()):
        with pytest.raises(ValueError):
            local(d, bad, 1.0, 8)
        with pytest.raises(ValueError):
            step(d, bad, 1.0, 8)
    p = torch.rand(16, 16, device=gpu)
    with pytest.raises(ValueError):
        local(d, p, 1.0, 8, mode="max")
    with pytest.raises(ValueError):
        step(d, p, 1.0, 8, origin=3)
    with pytest.raises(ValueError):
        step(d, p, 1.0, 8, grad_out=torch.zeros(1, 16, 15, device=gpu))
    for patch, origin in ((1, (0, 0)), (257, (0, 0)), (8, (8, 0)), (8, (0, -1)), (17, (0, 0)), (16, (1, 0))):
        with pytest.raises(_lib.Syn3rError):
            local(d, p, 1.0, patch, origin)
        with pytest.raises(_lib.Syn3rError):
            step(d, p, 1.0, patch, origin)


# ---------------------------------------------------------------- the trainer with the term on
@pytest.mark.parametrize("weights", [(0.0, 0.05), (0.05, 0.05)], ids=["local", "both"])
def test_explicit_step_equals_autograd_step(weights, gpu):
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    N, H, W = 3000, 72, 104
    w2c = np.eye(4, dtype=np.float32)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(5))
    _, K = _scene(N, H, W, 7, gpu)
    prior = _prior(H, W, K, gpu)
    res = {}
    for route, dlw in (("autograd", weights[1]), ("explicit", weights[1]), ("off", 0.0)):
        gm, K = _scene(N, H, W, 7, gpu)
        cam = Camera.from_w2c(w2c, K, H, W, image=target, data_device=gpu, cam_confidence=0.7, depth_image=prior)
        tr = GSTrainer(gm, [cam], OptimizationParams(iterations=1, depth_weight=weights[0], depth_local_weight=dlw, depth_patch_size=16))
        assert tr.depth_patch_origin(cam) == tr.depth_patch_origin(cam, 0)
        loss, _ = tr._autograd_step(cam) if route == "autograd" else tr._explicit_step(cam)
        res[route] = [float(loss.detach())] + [p.grad.detach().clone() for p in gm.parameters()]
    assert abs(res["explicit"][0] - res["autograd"][0]) < 1e-6
    for a, b in zip(res["explicit"][1:], res["autograd"][1:]):
        scale = float(b.abs().max()) + 1e-20
        assert float((a - b).abs().max()) <= 2e-5 * scale, (float((a - b).abs().max()), scale)
    # the term is in the loss and in the gradients
    assert res["off"][0] < res["explicit"][0]
    assert float((res["off"][1] - res["explicit"][1]).abs().max()) > 1e-3 * float(res["explicit"][1].abs().max())


def test_one_step_with_local_term_matches_oracle(gpu, measurements):
    """One training step with the patch-wise term against the fp64 oracle rasteriser + the differentiable restatement +
    torch.optim.Adam (bars as tests/test_depth_loss_gpu.py::test_one_step_with_depth_term_matches_oracle)."""
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    from tests.test_train_ops_gpu import _published_ssim
    N, H, W, PS = 400, 40, 56, 8
    gm, K = _scene(N, H, W, 3, gpu)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1))
    prior = _prior(H, W, K, gpu, seed=8)
    dw = 0.05
    cam = Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, image=target, data_device=gpu, cam_confidence=0.5, depth_image=prior)
    tr = GSTrainer(gm, [cam], OptimizationParams(iterations=1, depth_local_weight=dw, depth_patch_size=PS))
    origin = tr.depth_patch_origin(cam, 0)
    P = [p.detach().cpu().double().clone().requires_grad_(True) for p in gm.parameters()]   # xyz, sh, opac, scale, rot
    oc, _, od, _, _ = RO.rasterize(P[0], torch.exp(P[3]), torch.nn.functional.normalize(P[4]), torch.sigmoid(P[2]), P[1],
                                   torch.ones(N, dtype=torch.float64), cam.world_view_transform.cpu().double(),
                                   cam.full_proj_transform.cpu().double(), cam.camera_center.cpu().double(),
                                   math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2), H, W, torch.zeros(3, dtype=torch.float64), 3)
    photo = 0.5 * (0.8 * (oc - target.double()).abs().mean() + 0.2 * (1.0 - _published_ssim(oc, target.double())))
    dterm = R.ref_local_torch(od, prior.cpu().double(), dw, PS, origin)
    loss_o = photo + dterm
    opt = torch.optim.Adam([{"params": [P[0]], "lr": 1.6e-4}, {"params": [P[1]], "lr": 2.5e-3}, {"params": [P[2]], "lr": 5e-2},
                            {"params": [P[3]], "lr": 5e-3}, {"params": [P[4]], "lr": 1e-3}], eps=1e-15)
    loss_o.backward()
    loss_o, dterm = loss_o.detach(), dterm.detach()
    loss_e, _ = tr._explicit_step(cam)
    errs = []
    for a, b in zip(gm.parameters(), P):
        scale = float(b.grad.abs().max()) + 1e-20
        errs.append(float((a.grad.detach().cpu().double() - b.grad).abs().max()) / scale)
    measurements("depth_local_oracle_step", loss_hip=float(loss_e), loss_oracle=float(loss_o), dterm=float(dterm), grad_rel=errs)
    assert float(dterm) > 0.0
    assert abs(float(loss_e) - float(loss_o)) < 1e-4
    assert max(errs) < 5e-3, errs
    opt.step()
    for p_ in gm.parameters():
        p_.grad = None
    loss_h = tr.train_step(cam)
    assert torch.is_tensor(loss_h) and loss_h.is_cuda
    assert abs(float(loss_h) - float(loss_o)) < 1e-4
    for a, b in zip(gm.parameters(), P):
        d = (a.detach().cpu().double() - b.detach()).abs()
        assert (d > 1e-6).double().mean() < 2e-2


def test_weight_zero_leaves_the_step_unchanged(gpu, monkeypatch):
    """depth_local_weight = 0, with and without a prior on the camera: the explicit step's loss and the gradients it hands the
    rasteriser are bitwise those of a trainer without the option; depth_net runs once per camera, and only with a term on."""
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    seen = spy_rasterize_backward(monkeypatch)
    N, H, W = 2000, 48, 64
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(2))
    _, K = _scene(N, H, W, 4, gpu)
    prior = _prior(H, W, K, gpu)
    w2c = np.eye(4, dtype=np.float32)

    def run(opt, **cam_kw):
        gm, _ = _scene(N, H, W, 4, gpu)
        cam = Camera.from_w2c(w2c, K, H, W, image=target, data_device=gpu, **cam_kw)
        return GSTrainer(gm, [cam], opt), cam

    base = _step_bits(*run(OptimizationParams()), seen)
    assert base[0][2] is None
    for opt, kw in ((OptimizationParams(depth_local_weight=0.0, depth_patch_size=16), dict(depth_image=prior)),
                    (OptimizationParams(depth_local_weight=0.0, depth_patch_size=16), {}),
                    (OptimizationParams(depth_local_weight=0.05, depth_patch_size=16), {})):        # on, but no prior and no depth_net
        _same(base, _step_bits(*run(opt, **kw), seen))
    # with the global term on, weight 0 leaves ITS step unchanged too
    glob = _step_bits(*run(OptimizationParams(depth_weight=0.05), depth_image=prior), seen)
    _same(glob, _step_bits(*run(OptimizationParams(depth_weight=0.05, depth_local_weight=0.0, depth_patch_size=16), depth_image=prior), seen))
    calls = []

    def depth_net(img):
        calls.append(img.shape)
        return prior.clone()

    tr, cam = run(OptimizationParams(depth_local_weight=0.0))
    tr.depth_net = depth_net
    _same(base, _step_bits(tr, cam, seen))
    assert not calls and cam.depth_image is None
    tr, cam = run(OptimizationParams(depth_local_weight=0.05, depth_patch_size=16))
    tr.depth_net = depth_net
    on = _step_bits(tr, cam, seen)
    assert on[0][2] is not None and not torch.equal(on[0][0], base[0][0])
    _step_bits(tr, cam, seen)
    assert len(calls) == 1 and calls[0] == (3, H, W) and torch.equal(cam.depth_image, prior)
    # both terms on: one depth gradient buffer, the sum of the two
    both = _step_bits(*run(OptimizationParams(depth_weight=0.05, depth_local_weight=0.05, depth_patch_size=16), depth_image=prior), seen)
    want = glob[0][2].double() + on[0][2].double()
    assert float((both[0][2].double() - want).abs().max()) <= 1.2e-7 * float(want.abs().max())
    # a camera smaller than the patch names the option
    tr, cam = run(OptimizationParams(depth_local_weight=0.05, depth_patch_size=64), depth_image=prior)
    with pytest.raises(ValueError, match="depth_patch_size"):
        tr._explicit_step(cam)


def _quadrant_prior(disparity):
    """The true disparity under another affine map in each quadrant: consistent locally, not globally"""
    H, W = disparity.shape
    out = disparity.clone()
    for (ys, xs), (a, b) in zip(((slice(0, H // 2), slice(0, W // 2)), (slice(0, H // 2), slice(W // 2, W)),
                                 (slice(H // 2, H), slice(0, W // 2)), (slice(H // 2, H), slice(W // 2, W))),
                                ((1.0, 0.0), (0.4, 0.5), (2.5, 0.1), (0.7, 1.0))):
        out[ys, xs] = a * disparity[ys, xs] + b
    return out.contiguous()


def _mean_patch_corr(tr, cams, P):
    local, _, _ = _ops()
    rs = []
    with torch.no_grad():
        for c in cams:
            _, parts = local(tr.render_view(c)["depth"], c.depth_image, 1.0, P, return_parts=True)
            rs.append(float(parts[1]))
    return float(np.mean(rs))


def test_local_term_raises_the_patch_correlation(gpu, tmp_path, measurements):
    from syn3r_amd import launch
    P, res = 16, {}
    for dw in (0.0, 0.5):
        args = launch.parse(["--scenes", "synthetic:0", "--model_path", str(tmp_path / f"w{dw}"), "--iterations", "300"])
        sc = launch.synthetic_scene("synthetic:0", args, gpu)
        tr = sc["trainer"]
        cams = tr.scene.getTrainCameras()
        assert all(c.depth_image is not None and c.depth_image.shape == (72, 128) for c in cams)
        for c in cams:
            c.depth_image = _quadrant_prior(c.depth_image)
        tr.opt.depth_local_weight, tr.opt.depth_patch_size = dw, P
        r0 = _mean_patch_corr(tr, cams, P)
        tr.training(iterations=300, disable_densification=True)
        res[dw] = (r0, _mean_patch_corr(tr, cams, P))
    measurements("depth_local_correlation", r_start=res[0.5][0], r_end_on=res[0.5][1], r_end_off=res[0.0][1])
    print(f"mean patch Pearson at iteration 0: {res[0.5][0]:.5f}; after 300 iterations: term on {res[0.5][1]:.5f}, off {res[0.0][1]:.5f}")
    assert res[0.0][0] == res[0.5][0]
    assert res[0.5][1] > res[0.5][0]
    assert res[0.5][1] > res[0.0][1]
