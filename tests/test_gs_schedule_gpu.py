"""The published 3DGS schedule on the device: Adam with two rates inside a row (`syn3r_adam_step_multi_rows`) against
torch.optim.Adam over separate head / tail tensors, `FusedAdam`'s row-split groups, and the trainer's three rules (f_rest rate,
position-rate decay, progressive SH degree) through `train_step`, the density control and the launcher."""
import ctypes as C
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
# the project's own Adam tolerances (tests/test_train_ops_gpu.py: parameters; moments with their absolute floor of ~1 ulp(1))
P_TOL = dict(rtol=2e-6, atol=1e-7)
M_TOL = dict(rtol=1e-5, atol=2e-7)


def _rows(lib, L, dev, P, G, M1, V1, lrs, tails, rows, heads, epss, steps, count=None):
    """One `syn3r_adam_step_multi_rows` launch over the listed tensors; returns the status (the caller checks it)."""
    n = len(P) if count is None else count
    m = len(P)
    arr = lambda ts: (C.c_void_p * m)(*[t.data_ptr() for t in ts])
    return lib.syn3r_adam_step_multi_rows(n, arr(P), arr(G), arr(M1), arr(V1), (C.c_longlong * m)(*[p.numel() for p in P]),
                                          (C.c_float * m)(*lrs), (C.c_float * m)(*tails) if tails is not None else None,
                                          (C.c_int * m)(*rows), (C.c_int * m)(*heads), 0.9, 0.999, (C.c_float * m)(*epss),
                                          (C.c_int * m)(*steps), L.stream_ptr(dev))


def _torch_reference(tensors, steps, gen):
    """torch.optim.Adam(eps=1e-15) on the CPU over `tensors` = [(values [rows, row_len], lr, lr_tail, head_len)] with the head and
    the tail columns of every row held as two SEPARATE tensors with two rates (a plain tensor: head_len = row_len).  Returns the
    per-step gradients [step][tensor] and the final (param, exp_avg, exp_avg_sq) per tensor, re-assembled as [rows, row_len]."""
    parts, groups = [], []
    for x, lr, lr_tail, head in tensors:
        h, t = x[:, :head].clone().requires_grad_(True), x[:, head:].clone().requires_grad_(True)
        parts.append((h, t))
        groups.append({"params": [h], "lr": lr})
        if t.numel():
            groups.append({"params": [t], "lr": lr_tail})
    opt = torch.optim.Adam(groups, eps=1e-15)
    grads = []
    for it in range(steps):
        step_grads = []
        for (h, t), (x, _, _, head) in zip(parts, tensors):
            gr = torch.randn(x.shape, generator=gen) * (10.0 ** (-(it % 3)))
            if it == 1:
                gr.view(-1)[::5] = 0.0                     # zero gradients with eps = 1e-15 (the 0 / eps path)
            h.grad, t.grad = gr[:, :head].clone(), gr[:, head:].clone()
            step_grads.append(gr)
        opt.step()
        grads.append(step_grads)
    final = []
    for h, t in parts:
        st = lambda key: torch.cat([opt.state[h][key], opt.state[t][key] if t.numel() else torch.zeros_like(t)], dim=1)
        final.append((torch.cat([h.detach(), t.detach()], dim=1), st("exp_avg"), st("exp_avg_sq")))
    return grads, final


def _run_entry_against_torch(gpu, specs, seed):
    """specs: [(rows, row_len, head_len, split?)]: 5 steps of the new entry, ONE launch per step over all of them."""
    from syn3r_amd import _lib as L
    lib = L.load()
    gen = torch.Generator().manual_seed(seed)
    tensors = []
    for k, (rows, row_len, head, split) in enumerate(specs):
        lr = 2.5e-3 * (1 + k)
        tensors.append((torch.randn(rows, row_len, generator=gen), lr, lr / 20 if split else lr, head if split else row_len))
    grads, final = _torch_reference(tensors, 5, gen)
    P = [x.clone().to(gpu) for x, _, _, _ in tensors]
    M1, V1 = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
    for it in range(5):
        G = [g.to(gpu) for g in grads[it]]
        rc = _rows(lib, L, gpu, P, G, M1, V1, [t[1] for t in tensors], [t[2] for t in tensors],
                   [s[1] if s[3] else 0 for s in specs], [s[2] if s[3] else 0 for s in specs], [1e-15] * len(P), [it + 1] * len(P))
        L.check(rc, "adam_step_multi_rows")
    torch.cuda.synchronize()
    for (rp, rm, rv), p, m, v in zip(final, P, M1, V1):
        torch.testing.assert_close(p.cpu(), rp, **P_TOL)
        torch.testing.assert_close(m.cpu(), rm, **M_TOL)
        torch.testing.assert_close(v.cpu(), rv, **M_TOL)


# [N, M, 3] features: row_len = 3 M, head_len = 3.  (7, 1): all head; (5461, 16): 262 128 elements = 1023.9 blocks, no multiple of
# 256, and 48-float rows meet the block boundaries in every phase 16 k mod 48.  The last three are rows of 255 / 256 / 257 floats: the
# two sides of the kernel's switch between the reciprocal thread column (row_len <= 255) and the plain one (row_len >= 256)
@pytest.mark.parametrize("rows,row_len,head_len", [(1, 48, 3), (5, 12, 3), (7, 3, 3), (5461, 48, 3),
                                                   (9, 255, 100), (9, 256, 100), (9, 257, 100)])
def test_rows_entry_matches_torch_adam_on_separate_head_and_tail(rows, row_len, head_len, gpu):
    _run_entry_against_torch(gpu, [(rows, row_len, head_len, True)], seed=rows + row_len)


def test_rows_entry_mixes_split_and_plain_tensors_in_one_launch(gpu):
    """Two split tensors of different row_len (48 with a 3-float head; 300, above the block size, with a 7-float head) between
    three plain tensors of 1, 257 and 1000 elements."""
    _run_entry_against_torch(gpu, [(1, 1, 0, False), (100, 48, 3, True), (1, 257, 0, False), (11, 300, 7, True), (1, 1000, 0, False)],
                             seed=77)


def _ragged(gpu, seed):
    g = torch.Generator().manual_seed(seed)
    sizes = [48 * 1000, 3 * 1000, 1, 255, 257, 48 * 37, 513, 12345]
    mk = lambda n: torch.randn(n, generator=g).to(gpu)
    P = [mk(n) for n in sizes]; G = [mk(n) for n in sizes]; M1 = [mk(n).abs() * 0.1 for n in sizes]; V1 = [mk(n).abs() * 0.01 for n in sizes]
    lrs = [10.0 ** (-2 - (k % 3)) for k in range(len(sizes))]
    epss = [1e-15 if k % 2 else 1e-8 for k in range(len(sizes))]
    steps = [1 + 3 * k for k in range(len(sizes))]
    return sizes, P, G, M1, V1, lrs, epss, steps


def test_rows_entry_bitwise_equals_the_plain_entry(gpu):
    """Every row_len == 0 (lrs_tail not even passed), and split tensors whose two rates are equal: the bits of
    `syn3r_adam_step_multi` in the parameters and both moments."""
    from syn3r_amd import _lib as L
    lib = L.load()
    sizes, P, G, M1, V1, lrs, epss, steps = _ragged(gpu, 8)
    n = len(sizes)
    ref = [(p.clone(), m.clone(), v.clone()) for p, m, v in zip(P, M1, V1)]
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    rc = lib.syn3r_adam_step_multi(n, arr([r[0] for r in ref]), arr(G), arr([r[1] for r in ref]), arr([r[2] for r in ref]),
                                   (C.c_longlong * n)(*sizes), (C.c_float * n)(*lrs), 0.9, 0.999, (C.c_float * n)(*epss),
                                   (C.c_int * n)(*steps), L.stream_ptr(gpu))
    L.check(rc, "adam_step_multi")
    for rows, heads, tails in (([0] * n, [0] * n, None),
                               ([48, 3, 0, 0, 257, 48, 0, 0], [3, 3, 0, 0, 5, 0, 0, 0], lrs)):
        p2, m2, v2 = [p.clone() for p in P], [m.clone() for m in M1], [v.clone() for v in V1]
        L.check(_rows(lib, L, gpu, p2, G, m2, v2, lrs, tails, rows, heads, epss, steps), "adam_step_multi_rows")
        torch.cuda.synchronize()
        for (rp, rm, rv), p, m, v in zip(ref, p2, m2, v2):
            assert torch.equal(rp, p) and torch.equal(rm, m) and torch.equal(rv, v)


def test_fused_adam_without_split_keys_equals_per_tensor_launches(gpu):
    """`FusedAdam` whose groups carry no split key (and one whose row_len is 0) still takes `syn3r_adam_step_multi`: over three
    steps the bits of one `syn3r_adam_step` launch per tensor."""
    from syn3r_amd import _lib as L
    from syn3r_amd.gs.train_ops import FusedAdam
    lib = L.load()
    g = torch.Generator().manual_seed(9)
    sizes = [3 * 1000, 48 * 1000 + 7, 1, 255, 257, 4 * 1000, 1000, 513, 12345, 31]
    lrs = [10.0 ** (-2 - (k % 3)) for k in range(len(sizes))]
    hip_p = [torch.randn(n, generator=g).to(gpu).requires_grad_(True) for n in sizes]
    ref = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in hip_p]
    groups = [{"params": [p], "lr": lr} for p, lr in zip(hip_p, lrs)]
    groups[3].update(row_len=0, lr_tail=1.0, head_len=0)
    opt = FusedAdam(groups, eps=1e-15)
    for it in range(3):
        for (p, m, v), hp, lr in zip(ref, hip_p, lrs):
            hp.grad = torch.randn(hp.shape, generator=g).to(gpu)
            L.check(lib.syn3r_adam_step(L.ptr(p), L.ptr(hp.grad), L.ptr(m), L.ptr(v), p.numel(), lr, 0.9, 0.999, 1e-15, it + 1,
                                        L.stream_ptr(gpu)), "adam_step")
        opt.step()
    torch.cuda.synchronize()
    for (p, m, v), hp in zip(ref, hip_p):
        st = opt.state[hp]
        assert torch.equal(p, hp.detach()) and torch.equal(m, st["exp_avg"]) and torch.equal(v, st["exp_avg_sq"]) and st["step"] == 3


def test_rows_entry_refuses_bad_tables_and_leaves_the_parameters_alone(gpu):
    from syn3r_amd import _lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(3)
    mk = lambda n: torch.randn(n, generator=g).to(gpu)
    P, G, M1, V1 = [mk(480), mk(100)], [mk(480), mk(100)], [torch.zeros(480, device=gpu), torch.zeros(100, device=gpu)], \
        [torch.zeros(480, device=gpu), torch.zeros(100, device=gpu)]
    before = [t.clone() for t in P + M1 + V1]
    call = lambda rows, heads, **kw: _rows(lib, L, gpu, P, G, M1, V1, [1e-2, 1e-2], [1e-3, 1e-3], rows, heads, [1e-15] * 2, [1, 1], **kw)
    for rows, heads, word in (([48, 0], [49, 0], b"head_len"),             # head_len > row_len
                              ([48, 48], [3, 3], b"multiple"),             # 100 % 48 != 0
                              ([-1, 0], [0, 0], b"negative"),              # negative row_len
                              ([48, 0], [-1, 0], b"head_len")):            # negative head_len
        assert call(rows, heads) != 0
        assert word in lib.syn3r_last_error(), lib.syn3r_last_error()
    nine = [P[0]] * 9
    assert _rows(lib, L, gpu, nine, nine, nine, nine, [1e-2] * 9, [1e-3] * 9, [0] * 9, [0] * 9, [1e-15] * 9, [1] * 9) != 0
    assert b"count=9" in lib.syn3r_last_error()
    assert call([48, 0], [3, 0], count=0) != 0
    rc = _rows(lib, L, gpu, P, G, M1, V1, [1e-2, 1e-2], [1e-3, 1e-3], [48, 0], [3, 0], [1e-15] * 2, [1, 0])
    assert rc != 0 and b"1-based" in lib.syn3r_last_error()
    assert _rows(lib, L, gpu, P, G, M1, V1, [1e-2, 1e-2], None, [48, 0], [3, 0], [1e-15] * 2, [1, 1]) != 0      # a split without lrs_tail
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, P + M1 + V1))
    L.check(call([48, 0], [3, 0]), "adam_step_multi_rows")                 # and the good table of the same tensors runs
    torch.cuda.synchronize()
    assert not torch.equal(before[0], P[0]) and not torch.equal(before[1], P[1])


def test_fused_adam_row_split_groups_match_torch_groups(gpu):
    """Ten groups = two launches (8 + 2); a split group in each (48-float rows with a 3-float head; 12-float rows with a 3-float
    head).  Three steps against torch.optim.Adam over ten-plus-two groups."""
    from syn3r_amd.gs.train_ops import FusedAdam
    gen = torch.Generator().manual_seed(10)
    shapes = [(3000, 1), (1001, 48), (1, 1), (1, 255), (1, 257), (1000, 4), (1000, 1), (1, 513), (1, 12345), (31, 12)]
    split = {1: 3, 9: 3}
    lrs = [10.0 ** (-2 - (k % 3)) for k in range(len(shapes))]
    tensors = [(torch.randn(s, generator=gen), lr, lr / 20 if k in split else lr, split.get(k, s[1]))
               for k, (s, lr) in enumerate(zip(shapes, lrs))]
    grads, final = _torch_reference(tensors, 3, gen)
    hip_p = [x.clone().to(gpu).requires_grad_(True) for x, _, _, _ in tensors]
    groups = [{"params": [p], "lr": lr} for p, lr in zip(hip_p, lrs)]
    for k, head in split.items():
        groups[k].update(lr_tail=lrs[k] / 20, row_len=shapes[k][1], head_len=head)
    opt = FusedAdam(groups, eps=1e-15)
    for it in range(3):
        for hp, gr in zip(hip_p, grads[it]):
            hp.grad = gr.to(gpu)
        opt.step()
    for (rp, rm, rv), hp in zip(final, hip_p):
        torch.testing.assert_close(hp.detach().cpu(), rp, **P_TOL)
        torch.testing.assert_close(opt.state[hp]["exp_avg"].cpu(), rm, **M_TOL)
        torch.testing.assert_close(opt.state[hp]["exp_avg_sq"].cpu(), rv, **M_TOL)
    assert groups[1]["row_len"] == 48 and opt.param_groups[9]["lr_tail"] == lrs[9] / 20


# ---------------------------------------------------------------------------------------------- the trainer
N, H, W = 300, 40, 64


def _trainer(gpu, opt, active_sh_degree=None, second_camera=False):
    from oracle import raster_oracle as RO
    from syn3r_amd.gs import Camera, GaussianModel, GSTrainer
    m, s, q, o, sh = RO.synthetic_gaussians(N, seed=5, log_scale_mean=np.log(0.08))
    logit = torch.log(o.clamp(1e-3, 1 - 1e-3) / (1 - o.clamp(1e-3, 1 - 1e-3)))
    gm = GaussianModel(m, torch.log(s), q, logit, sh, device=gpu, active_sh_degree=active_sh_degree)
    f = W / (2 * math.tan(math.radians(30)))
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], dtype=np.float32)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(6))
    cams = [Camera.from_w2c(np.eye(4, dtype=np.float32), K, H, W, image=target, data_device=gpu)]
    if second_camera:                       # never rendered: it gives `cameras_extent()` a value other than the one-camera 1.0
        p = np.eye(4, dtype=np.float32)
        p[0, 3] = 0.3
        cams.append(Camera.from_w2c(p, K, H, W, image=target, data_device=gpu))
    return GSTrainer(gm, cams, opt), gm, cams[0]


def test_first_explicit_step_moves_f_dc_by_lr_and_f_rest_by_a_twentieth(gpu, measurements):
    """Adam's first update is lr g / (|g| + eps): with `feature_rest_lr_div = 20` every SH coefficient with a gradient moves by
    feature_lr in row 0 of its Gaussian (columns 0..2 of the 48-float row) and by feature_lr / 20 in rows 1..15, a coefficient
    without one keeps its bits.  The coefficients start at ZERO here, so the parameter's own rounding (half an ulp of an O(1) value
    is 2e-4 of a 1.25e-4 step) stays out of the difference and what is left is the update's handful of fp32 roundings."""
    from syn3r_amd.gs import OptimizationParams
    opt = OptimizationParams(iterations=1, feature_rest_lr_div=20.0)
    tr, gm, cam = _trainer(gpu, opt, active_sh_degree=3)
    with torch.no_grad():
        gm._features.zero_()
        gm._xyz[:10, 2] = -5.0                                      # ten Gaussians behind the camera: culled, exact zero gradient
    grp = tr.optimizer.param_groups[1]
    assert (grp["lr"], grp["lr_tail"], grp["row_len"], grp["head_len"]) == (opt.feature_lr, opt.feature_lr / 20.0, 48, 3)
    before = gm._features.detach().clone()
    tr.train_step(cam, explicit=True)
    grad = gm._features.grad.detach().double().cpu()
    delta = (gm._features.detach() - before).double().cpu()
    assert grad.shape == (N, 16, 3)
    nz = grad != 0
    assert 0.05 < float(nz.double().mean()) and not bool(nz[:10].any())
    assert torch.equal(gm._features.detach()[~nz.to(gpu)], before[~nz.to(gpu)])                  # bit-unchanged
    lr = torch.full_like(grad, opt.feature_lr / 20.0)
    lr[:, 0, :] = opt.feature_lr
    expect = -lr * grad / (grad.abs() + 1e-15)
    rel = ((delta - expect).abs() / expect.abs().clamp_min(1e-300))[nz]
    measurements("gs_schedule_first_step", max_rel=float(rel.max()), min_abs_grad=float(grad.abs()[nz].min()), nonzero=int(nz.sum()))
    print("first step: max rel", float(rel.max()), "min |g|", float(grad.abs()[nz].min()), "nonzero", int(nz.sum()))
    assert float(rel.max()) <= 1e-5
    assert bool((delta[:, 0, :][nz[:, 0, :]].abs() > 0.99 * opt.feature_lr).all())
    assert bool((delta[:, 1:, :][nz[:, 1:, :]].abs() < 1.01 * opt.feature_lr / 20.0).all())


@pytest.mark.parametrize("explicit,steps", [(True, 14), (False, 5)])
def test_schedule_run_decays_the_position_rate_and_raises_the_degree(explicit, steps, gpu):
    from syn3r_amd.gs import OptimizationParams
    from syn3r_amd.gs.trainer import expon_lr
    opt = OptimizationParams(iterations=steps, sh_degree_interval=4, position_lr_final=1.6e-4 / 100, position_lr_max_steps=12,
                             spatial_lr_scale=None)
    tr, gm, cam = _trainer(gpu, opt, active_sh_degree=0, second_camera=True)
    extent = tr.cameras_extent()
    assert abs(extent - 0.15 * 1.1) < 1e-6 and tr.spatial_lr_scale == extent
    initial = gm._features.detach().clone()
    xyz_group = tr.optimizer.param_groups[0]
    assert gm.active_sh_degree == 0 and xyz_group["lr"] == opt.position_lr
    for step in range(1, steps + 1):
        d = gm.active_sh_degree                                    # the degree THIS step renders with
        assert d == min(3, (step - 1) // 4)
        xyz_before = gm._xyz.detach().clone()
        tr.train_step(cam, explicit=explicit)
        assert gm.active_sh_degree == min(3, step // 4)
        # the rate the step was taken with (written before the optimiser step, from the loop's 1-based counter)
        want = extent * expon_lr(step, opt.position_lr, opt.position_lr_final, 0, opt.position_lr_delay_mult, 12)
        assert xyz_group["lr"] == want and tr.iteration == step
        if step == 1:                                              # Adam's first step: the coordinates that moved moved by that rate,
            dx = float((gm._xyz.detach() - xyz_before).abs().max())        # seen through one rounding of the coordinate itself
            ulp = float(torch.finfo(torch.float32).eps * xyz_before.abs().max())
            assert want * 0.99 - ulp <= dx <= want * 1.01 + ulp, (dx, want, ulp)
        rows = (d + 1) ** 2
        feats = gm._features.detach()
        assert torch.equal(feats[:, rows:], initial[:, rows:])     # inactive rows: exact zero gradient, zero moments, no move
        assert not torch.equal(feats[:, :rows], initial[:, :rows])
        if d > 0:
            assert not torch.equal(feats[:, d * d:rows], initial[:, d * d:rows])      # the band switched on last has moved
    if steps >= 12:
        assert xyz_group["lr"] == extent * opt.position_lr_final   # at and beyond max_steps
    assert tr.update_learning_rate(0) == extent * opt.position_lr


def test_density_control_keeps_the_row_split(gpu):
    """`test_training_with_density_control_changes_the_set_and_keeps_fitting`'s schedule at its N with the f_rest rate on: clone /
    split / prune swap the features tensor inside its group, the keys stay, whole rows stay."""
    from syn3r_amd.gs import Camera, GSTrainer, OptimizationParams
    from tests.test_trainer_gpu import make_scene
    n0, h, w = 1500, 64, 96
    gt, K = make_scene(n0, h, w, 11, gpu)
    cam0 = Camera.from_w2c(np.eye(4, dtype=np.float32), K, h, w, data_device=gpu)
    target = GSTrainer(gt, [cam0]).render_view(cam0)["render"].detach()
    gm, _ = make_scene(n0, h, w, 12, gpu)
    cam = Camera.from_w2c(np.eye(4, dtype=np.float32), K, h, w, image=target, data_device=gpu)
    opt = OptimizationParams(iterations=120, position_lr=2e-3, densify_from_iter=10, densification_interval=20,
                             opacity_reset_interval=1000, densify_grad_threshold=3e-4, prune_min_opacity=0.02, feature_rest_lr_div=20.0)
    tr = GSTrainer(gm, [cam], opt)
    first = float(tr.train_step(cam))
    last = tr.training(0, 0)
    n_now = gm._xyz.shape[0]
    grp = tr.optimizer.param_groups[1]
    assert n_now != n0 and gm._features.shape == (n_now, 16, 3)
    assert grp["params"][0] is gm._features and (grp["row_len"], grp["head_len"], grp["lr_tail"]) == (48, 3, opt.feature_lr / 20.0)
    assert gm._features.numel() % grp["row_len"] == 0 and tr.optimizer.state[gm._features]["exp_avg"].shape == gm._features.shape
    before = gm._features.detach().clone()
    tr.densify = False
    tr.train_step(cam)                                              # a further step runs through the split launch
    moved = (gm._features.detach() - before).abs()
    assert float(moved.max()) > 0 and bool(torch.isfinite(gm._features).all())
    assert np.isfinite(last) and last < first, (first, last)
    assert tr.truncated_renders == 0


def test_launcher_child_process_with_the_published_schedule(gpu, tmp_path):
    r = subprocess.run([sys.executable, "-m", "syn3r_amd.launch", "--scenes", "synthetic:0:500", "--model_path", str(tmp_path),
                        "--gs_schedule", "published", "--iterations", "30", "--refine_cycle_num", "0", "--percent_dense", "0.001",
                        "--diffusion_type", "2PassProbUncertain", "--densify_type", "interpolate_gs_v2"],
                       capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert "psnr" in lines[0] and "mean over finished scenes" in lines[-1] and len(lines) == 3, r.stdout
    rec = [float(v) for v in lines[1].split()[:9]]
    assert rec[0] == 0.0 and rec[8] == 1.0 and math.isfinite(rec[1]) and rec[1] > 0.0, rec
    assert "--percent_dense" not in r.stderr                       # (the notice about ignored flags lists what it dropped)
