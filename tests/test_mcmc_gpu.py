"""3DGS-MCMC density control on the GPU: the kernels of csrc/mcmc.hip through the operators of `train_ops` against the float64 /
Python-integer restatement tests/mcmc_ref.py, and the trainer's `OptimizationParams.mcmc` on the synthetic scene of
tests/trainer_launches.py.  Every operator that allocates runs under tests/poison.py.

The grid of the per-Gaussian kernels, restated (csrc/mcmc.hip `blocks_for`): one Gaussian per thread and trip, 256 threads,
blocks = min(ceil(n / 256), 2048), trips = ceil(n / (256 blocks)).

The bounds.  u = 2^-24; a function documented at 1 ulp (the HIP math API's single-precision table: logf, sqrtf, cospif, sinpif, expf)
has a relative error of at most 2u, an fp32 operation u.

* noise: eps_j = sqrtf(-2 logf(U)) * cospif(2 V) with U, V and 2 V exact: logf 2u, halved by the root to u, sqrtf 2u, the pi-function
  2u, the product u = 6u relative to |eps_j|.  Everything after eps is fp64 on the fp32 inputs (about forty operations at 2^-53) and
  one rounding to fp32, u: 7u, and c = 8 leaves 1u for the second-order terms and the fp64 arithmetic.  r_j is the Box-Muller radius
  of eps_j, so an error of the pi-function counts in units of the radius.  A result below the fp32 normal range cannot be closer
  than one subnormal step, whatever computes it: + 2^-149 (opacity 0.999 has gate(o) = e^-99.4 = 7e-44).
* regularisers: the sums are t fp32 additions per thread (t = trips for the opacity, 3 trips for the scales), six for the wave, two
  for the block, then fp64; act_sigmoid is expf 2u + an addition + a division = 4u, expf 2u.  Values: 2 (t + 10) u of the sum of
  terms, all positive (the grad_A bound of tests/test_exposure_gpu.py).  Gradients: |d(o (1 - o))| <= 6u o, the weight and the product
  u each, the addition u of the result.
* weights: 0.5 for rintf + 65536 * 4u o for act_sigmoid (the product with 2^16 is exact).
* relocation: fp64; the 51-term alternating sum loses (sum |term| / |sum|) x 128 x 2^-53 (one rounding per term, binomial, power
  and root, with a 2x margin), the results are rounded to fp32 once each (and the log-scale once more when the difference is added)."""
import functools
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import mcmc_ref as R  # noqa: E402
import trainer_launches as TL  # noqa: E402
from poison import poisoned  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
THREADS, MAX_BLOCKS = 256, 2048
BIG = THREADS * MAX_BLOCKS + 37          # just past a full capped grid trip: the grid-stride loop takes a second one
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, BIG]
SCALE = 80.0                             # mcmc_noise_lr 5e5 x position_lr 1.6e-4
C_NOISE = 8
DEAD = float(np.float32(math.log(0.005 / 0.995)))
MIN_OP = float(np.float32(0.005))


def trips(n: int) -> int:
    blocks = min(max(-(-n // THREADS), 1), MAX_BLOCKS)
    return -(-n // (THREADS * blocks))


@functools.lru_cache(maxsize=None)
def master():
    """Seeded raw parameters of the largest size (CPU fp32); size n uses the first n rows, so an index has the same inputs in every
    size.  Rotations random, log-scales in [-6, 1], opacities log-uniform in [1e-4, 0.999]"""
    g = torch.Generator().manual_seed(20)
    rot = torch.randn(BIG, 4, generator=g)
    ls = torch.rand(BIG, 3, generator=g) * 7.0 - 6.0
    o = torch.exp(torch.rand(BIG, generator=g).double() * (math.log(0.999) - math.log(1e-4)) + math.log(1e-4))
    logit = torch.log(o / (1.0 - o)).float()
    return rot, ls, logit


@functools.lru_cache(maxsize=None)
def noise_ref(n: int, seed: int, step: int):
    rot, ls, logit = master()
    return R.noise(ls[:n].numpy(), rot[:n].numpy(), logit[:n].numpy(), SCALE, seed, step)


def _run_noise(n, seed, step, dev):
    from syn3r_amd.gs import train_ops as T
    rot, ls, logit = (t[:n].to(dev) for t in master())
    xyz = torch.zeros(n, 3, device=dev)
    T.mcmc_noise(xyz, ls, rot, logit, SCALE, seed, step)
    return xyz


def _ratio(got, ref, bound) -> float:
    """largest |got - ref| / bound (0 / 0 counts as 0)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("n", SIZES)
def test_noise_against_float64(n, gpu, measurements):
    worst = 0.0
    for seed, step in ((0, 1), (0, 2), ((0xC0FFEE << 32) | 5, 1), ((0xC0FFEE << 32) | 5, 30_000)):
        ref, mag = noise_ref(n, seed, step)
        got = _run_noise(n, seed, step, gpu).cpu().numpy()
        assert np.isfinite(got).all()
        r = _ratio(got, ref, C_NOISE * EPS * mag + 2.0 ** -149)
        worst = max(worst, r)
        assert r <= 1.0, f"noise n={n} seed={seed} step={step}: largest error / bound = {r:.3f}"
    measurements("mcmc_noise", n=n, ratio=worst)
    print(f"mcmc_noise n={n}: largest error {worst:.3f} of the bound (c = {C_NOISE})")


def test_noise_is_repeatable_and_a_function_of_the_index(gpu):
    a, b = _run_noise(257, 3, 7, gpu), _run_noise(257, 3, 7, gpu)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    other_step, other_seed = _run_noise(257, 3, 8, gpu), _run_noise(257, 4, 7, gpu)
    live = a.abs().amax(dim=1) > 1e-30                                # (a closed gate leaves a few subnormal steps or zero)
    assert int(live.sum()) > 100
    assert bool((a[live] != other_step[live]).any(dim=1).all()) and bool((a[live] != other_seed[live]).any(dim=1).all())
    # the same index draws the same numbers whatever n (and with it the grid) is
    for n in (1, 63, 64, 256):
        assert torch.equal(_run_noise(n, 3, 7, gpu).view(torch.int32), a[:n].view(torch.int32))
    big = _run_noise(BIG, 3, 7, gpu)
    assert torch.equal(big[:257].view(torch.int32), a.view(torch.int32))
    # in place: the noise is ADDED to what xyz holds (one rounding of the fp64 sum)
    from syn3r_amd.gs import train_ops as T
    rot, ls, logit = (t[:257].to(gpu) for t in master())
    start = torch.randn(257, 3, generator=torch.Generator().manual_seed(1)).to(gpu)
    xyz = start.clone()
    T.mcmc_noise(xyz, ls, rot, logit, SCALE, 3, 7)
    ref = start.cpu().double().numpy() + noise_ref(257, 3, 7)[0]
    assert _ratio(xyz.cpu().numpy(), ref, C_NOISE * EPS * noise_ref(257, 3, 7)[1] + EPS * np.abs(ref) + 2.0 ** -149) <= 1.0
    # scale 0 leaves every bit
    T.mcmc_noise(xyz, ls, rot, logit, 0.0, 3, 7)
    T.mcmc_noise(start, ls, rot, logit, SCALE, 3, 7)
    assert torch.equal(xyz.view(torch.int32), start.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ regularisers
@pytest.mark.parametrize("n", SIZES)
def test_regularisers_against_float64(n, gpu, monkeypatch, measurements):
    from syn3r_amd.gs import train_ops as T
    _, ls, logit = master()
    ls, logit = ls[:n], logit[:n]
    g = torch.Generator().manual_seed(n)
    pre_o, pre_s = torch.randn(n, generator=g), torch.randn(n, 3, generator=g)          # the gradients are ADDED to this pattern
    reg_o, reg_s = 0.01, 0.03
    values, go, gs = R.regularisers(logit.numpy(), ls.numpy(), float(np.float32(reg_o)), float(np.float32(reg_s)))
    outs = []
    for byte in (0xFF, 0x3C):
        with poisoned(monkeypatch, byte):
            grad_o, grad_s = pre_o.to(gpu), pre_s.to(gpu)
            out = T.mcmc_reg_step(logit.to(gpu), ls.to(gpu), reg_o, reg_s, grad_o, grad_s)
            outs.append((out.cpu(), grad_o.cpu(), grad_s.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))                    # repeatable, whatever the workspace held
    out, grad_o, grad_s = outs[0]
    t = trips(n)
    bound = np.array([2 * (t + 10), 2 * (3 * t + 10)]) * EPS * values
    r_v = _ratio(out.numpy(), values, bound)
    o, e = R.sigmoid(logit.numpy()), np.exp(ls.double().numpy())
    exp_o, exp_s = pre_o.double().numpy() + go, pre_s.double().numpy() + gs
    r_o = _ratio(grad_o.numpy(), exp_o, EPS * (np.abs(exp_o) + 10 * reg_o / n * o))
    r_s = _ratio(grad_s.numpy(), exp_s, EPS * (np.abs(exp_s) + 6 * reg_s / (3 * n) * e))
    measurements("mcmc_reg", n=n, value_ratio=r_v, grad_opacity_ratio=r_o, grad_scale_ratio=r_s)
    print(f"mcmc_reg n={n}: values {r_v:.3f}, grad_opacity {r_o:.3f}, grad_log_scales {r_s:.3f} of their bounds (trips = {t})")
    assert r_v <= 1.0 and r_o <= 1.0 and r_s <= 1.0, (r_v, r_o, r_s)


def test_regularisers_planted_elements_are_summed_exactly(gpu):
    """Logits and log-scales of -200 (sigmoid and exp are exactly 0 in fp32) except at the first and the last Gaussian and on both
    sides of a wave, block and grid-trip boundary, where the logit is 0 (opacity 1/2) and the first two log-scales are 0 (scale 1):
    every partial sum is a small multiple of 1/2, exact in fp32, so the two values must EQUAL the float64 result, and the gradients
    are the pre-filled pattern everywhere else."""
    from syn3r_amd.gs import train_ops as T
    n = BIG
    per_trip = THREADS * MAX_BLOCKS
    assert trips(n) == 2 and per_trip < n
    edges = [64, THREADS, (MAX_BLOCKS - 1) * THREADS, per_trip, per_trip + 1, n - 1]
    plants = sorted({0, n - 1} | {e - 1 for e in edges} | set(edges))
    idx = torch.tensor(plants, device=gpu)
    logit, ls = torch.full((n,), -200.0, device=gpu), torch.full((n, 3), -200.0, device=gpu)
    logit[idx] = 0.0
    ls[idx, 0] = 0.0
    ls[idx, 1] = 0.0
    pre_o = torch.arange(n, device=gpu, dtype=torch.float32) % 7 - 3.0
    pre_s = (torch.arange(3 * n, device=gpu, dtype=torch.float32) % 5 - 2.0).view(n, 3)
    grad_o, grad_s = pre_o.clone(), pre_s.clone()
    reg_o, reg_s = np.float32(0.01), np.float32(0.03)
    out = T.mcmc_reg_step(logit, ls, float(reg_o), float(reg_s), grad_o, grad_s).cpu().numpy()
    k = len(plants)
    expect = np.array([np.float32(0.5 * k * (float(reg_o) / n)), np.float32(2.0 * k * (float(reg_s) / (3.0 * n)))], dtype=np.float32)
    assert np.array_equal(out, expect), (out.tolist(), expect.tolist())
    changed_o = (grad_o != pre_o).nonzero().view(-1).cpu().tolist()
    changed_s = (grad_s != pre_s).any(dim=1).nonzero().view(-1).cpu().tolist()
    # (pattern value 0 + a gradient of 1e-9 changes; a pattern value of 1 or more absorbs it: compare where the pattern is 0)
    zero_o = [p for p in plants if p % 7 == 3]
    assert set(changed_o) <= set(plants) and set(zero_o) <= set(changed_o)
    assert set(changed_s) <= set(plants)
    go = np.float32(float(reg_o) / n)
    for p in zero_o:
        assert float(grad_o[p]) == float(np.float32(go * np.float32(0.25)))


# ------------------------------------------------------------------------------------------------------------------ weights
def test_weights(gpu, monkeypatch):
    from syn3r_amd.gs import train_ops as T
    _, _, logit = master()
    n = 70_001
    dead32 = np.float32(DEAD)
    edge = torch.tensor([dead32, np.nextafter(dead32, np.float32(0)), np.nextafter(dead32, np.float32(-10)), -100.0, 100.0, 0.0, 20.0],
                        dtype=torch.float32)
    lg = torch.cat([edge, logit[:n - edge.numel()]])
    with poisoned(monkeypatch, 0xFF):
        w = T.mcmc_weights(lg.to(gpu), DEAD)
    assert w.dtype == torch.int32 and w.shape == (n,)
    w = w.cpu().numpy().astype(np.int64)
    value, dead = R.weights(lg.numpy(), DEAD)
    assert dead[0] and not dead[1] and dead[2] and int(dead.sum()) > 1000 and int((~dead).sum()) > 1000
    assert np.array_equal(w == 0, dead)
    live = ~dead
    assert int(w[live].min()) >= 328 and int(w.max()) == 65536 and w[4] == 65536 and w[5] == 32768
    r = _ratio(w[live], value[live], 0.5 + 65536.0 * 4 * EPS * value[live] / 65536.0)
    print(f"mcmc_weights: largest error {r:.3f} of the bound")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------------------------ sampling
def _sample_case(name: str):
    rng = np.random.default_rng(5)
    if name.startswith("single-"):
        n = 4097
        w = np.zeros(n, dtype=np.int64)
        w[{"first": 0, "middle": 2048, "last": n - 1}[name.split("-")[1]]] = 40000
        return w
    if name == "ones":
        return np.ones(1000, dtype=np.int64)
    if name == "zero-runs":                   # runs of zeros between positives, a whole chunk of zeros among them
        w = rng.integers(328, 65537, size=3 * 4096 + 5)
        for a, b in ((0, 3), (10, 400), (4000, 4100), (4096, 8192), (12000, 12200), (12290, 12293)):
            w[a:b] = 0
        return w
    if name in ("4095", "4096", "4097"):
        w = rng.integers(0, 65537, size=int(name))
        w[rng.random(int(name)) < 0.3] = 0
        return w
    if name == "past-2^32":
        return np.full(70_000, 65536, dtype=np.int64)
    if name == "past-2^32-holes":
        w = np.full(70_000, 65536, dtype=np.int64)
        w[rng.integers(0, 70_000, size=200)] = 0
        return w
    if name == "all-dead":
        return np.zeros(4097, dtype=np.int64)
    raise KeyError(name)


SAMPLE_CASES = ["single-first", "single-middle", "single-last", "ones", "zero-runs", "4095", "4096", "4097", "past-2^32",
                "past-2^32-holes", "all-dead"]


@pytest.mark.parametrize("name", SAMPLE_CASES)
def test_sampling_is_exact(name, gpu, monkeypatch):
    from syn3r_amd.gs import train_ops as T
    w = _sample_case(name)
    n = len(w)
    if name.startswith("past"):
        assert int(w.sum()) > 2 ** 32
    wd = torch.tensor(w, dtype=torch.int32, device=gpu)
    seed, step = (7 << 32) | 123, 4100
    for m_extra, byte in ((0, 0xFF), (1, 0x3C), (300, 0xFF)):
        with poisoned(monkeypatch, byte):
            src, counts = T.mcmc_sample(wd, m_extra, seed, step)
        assert src.shape == (n + m_extra,) and counts.shape == (n,) and src.dtype == torch.int32 and counts.dtype == torch.int32
        src, counts = src.cpu().numpy().astype(np.int64), counts.cpu().numpy().astype(np.int64)
        ref_src, ref_counts = R.sample(w, m_extra, seed, step)
        assert np.array_equal(src, ref_src), (name, m_extra, int((src != ref_src).sum()))
        assert np.array_equal(counts, ref_counts)
        assert np.array_equal(counts, np.bincount(src[src >= 0], minlength=n))
        if name == "all-dead":
            assert bool((src == -1).all()) and int(counts.sum()) == 0
        else:
            assert bool((src[:n][w > 0] == -1).all()) and bool((src[:n][w == 0] >= 0).all()) and bool((src[n:] >= 0).all())
            assert bool((w[src[src >= 0]] > 0).all())


# ------------------------------------------------------------------------------------------------------------------ relocation
OPACITIES = (0.005, 0.1, 0.5, 0.9, 0.99, 0.999999)
COUNTS = (1, 2, 9, 50, 51, 200)


def _relocation_case(dev):
    """Rows [0, 36): destinations whose source index is LARGER; [36, 72): the 36 sources, one per (opacity, count); [72, 108): a
    second destination of every source, whose source index is SMALLER; [108, 120): bystanders"""
    S = len(OPACITIES) * len(COUNTS)
    n = 3 * S + 12
    g = torch.Generator().manual_seed(9)
    xyz, feat, rot = torch.randn(n, 3, generator=g), torch.randn(n, 4, 3, generator=g), torch.randn(n, 4, generator=g)
    ls = torch.rand(n, 3, generator=g) * 7.0 - 6.0
    logit = torch.randn(n, generator=g)
    src, counts = torch.full((n,), -1, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    pairs = [(o, c) for o in OPACITIES for c in COUNTS]
    for k, (o, c) in enumerate(pairs):
        logit[S + k] = math.log(o / (1.0 - o))
        counts[S + k] = c
        src[k] = S + k
        src[2 * S + k] = S + k
    params = [t.to(dev) for t in (xyz, feat, logit, ls, rot)]
    moments = [torch.randn(p.shape, generator=g).to(dev) for p in (xyz, xyz, feat, feat, logit, logit, ls, ls, rot, rot)]
    return S, n, pairs, src.to(dev), counts.to(dev), params, moments


@pytest.mark.parametrize("null_moments", ["none", "all", "some"])
def test_relocation_against_float64(null_moments, gpu, measurements):
    from syn3r_amd.gs import train_ops as T
    S, n, pairs, src, counts, params, moments = _relocation_case(gpu)
    if null_moments == "all":
        moments = [None] * 10
    elif null_moments == "some":
        moments = [m if k in (0, 1, 4, 9) else None for k, m in enumerate(moments)]
    old = [p.clone() for p in params]
    old_m = [None if m is None else m.clone() for m in moments]
    xyz, feat, logit, ls, rot = params
    T.mcmc_relocate(src, counts, xyz, feat, logit, ls, rot, moments, MIN_OP)
    torch.cuda.synchronize()
    o_xyz, o_feat, o_logit, o_ls, o_rot = (t.cpu() for t in old)
    xyz, feat, logit, ls, rot = (t.cpu() for t in params)
    worst_l, worst_s = 0.0, 0.0
    for k, (o_nominal, c) in enumerate(pairs):
        s, d_hi, d_lo = S + k, k, 2 * S + k
        o = float(R.sigmoid(np.float64(o_logit[s].item())))                              # the opacity of the fp32 logit
        on, factor, cond = R.relocation(o, c, MIN_OP)
        logit_ref, dls = math.log(on / (1.0 - on)), math.log(factor)
        b_logit = EPS * abs(logit_ref) + 1e-8
        worst_l = max(worst_l, abs(float(logit[s]) - logit_ref) / b_logit)
        for j in range(3):
            ls_ref = float(o_ls[s, j]) + dls
            b = EPS * (abs(dls) + abs(ls_ref)) + cond * 128 * 2.0 ** -53
            worst_s = max(worst_s, abs(float(ls[s, j]) - ls_ref) / b)
        # the two destinations: copies of the source's OLD position, rotation and features, with the source's new logit; their
        # log-scales are their source's OLD ones plus the same difference (the source's own bits where the old log-scales agree)
        for d in (d_hi, d_lo):
            assert torch.equal(xyz[d], o_xyz[s]) and torch.equal(rot[d], o_rot[s]) and torch.equal(feat[d], o_feat[s])
            assert torch.equal(logit[d].view(torch.int32), logit[s].view(torch.int32))
            assert torch.equal(ls[d].view(torch.int32), ls[s].view(torch.int32))
        assert torch.equal(xyz[s], o_xyz[s]) and torch.equal(rot[s], o_rot[s]) and torch.equal(feat[s], o_feat[s])
    measurements("mcmc_relocate", logit_ratio=worst_l, log_scale_ratio=worst_s)
    print(f"mcmc_relocate: logit {worst_l:.3f}, log-scales {worst_s:.3f} of their bounds")
    assert worst_l <= 1.0 and worst_s <= 1.0, (worst_l, worst_s)
    # bystanders keep every bit; the moments of touched rows are zero, the others keep their bits
    for new, was in zip((xyz, feat, logit, ls, rot), (o_xyz, o_feat, o_logit, o_ls, o_rot)):
        assert torch.equal(new[3 * S:].view(torch.int32), was[3 * S:].view(torch.int32))
    for m, was in zip(moments, old_m):
        if m is not None:
            assert bool((m[:3 * S] == 0).all()) and torch.equal(m[3 * S:].view(torch.int32), was[3 * S:].view(torch.int32))
    # opacity of every touched row: above the dead threshold, below 1
    assert bool((logit[:3 * S] >= np.float32(math.log(MIN_OP / (1 - MIN_OP))) - 1e-6).all()) and bool(torch.isfinite(logit).all())


def test_relocation_after_sampling_leaves_no_dead_gaussian(gpu, monkeypatch):
    """weights -> sample -> relocate as the control chains them: every dead row becomes alive, bit-repeatably"""
    from syn3r_amd.gs import mcmc as M
    from syn3r_amd.gs import train_ops as T
    rot, ls, logit = (t[:5000] for t in master())
    feat = torch.randn(5000, 16, 3, generator=torch.Generator().manual_seed(2))
    results = []
    for byte in (0xFF, 0x3C):
        with poisoned(monkeypatch, byte):
            p = [t.clone().to(gpu) for t in (torch.zeros(5000, 3) + torch.arange(5000.0)[:, None], feat, logit, ls, rot)]
            w = T.mcmc_weights(p[2], M.dead_logit(0.005))
            dead = w == 0
            assert 100 < int(dead.sum()) < 4900
            src, counts = T.mcmc_sample(w, 0, 11, 600)
            T.mcmc_relocate(src, counts, *p, [None] * 10, M.clamp_opacity(0.005))
            assert int((T.mcmc_weights(p[2], M.dead_logit(0.005)) == 0).sum()) == 0
            assert torch.equal(p[0][dead][:, 0].long(), src[dead].long())                # a dead row sits where its source is
            results.append(p)
    for a, b in zip(*results):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ the trainer
def make_trainer(dev, **fields):
    """The scene of tests/trainer_launches.py (300 Gaussians, 33 x 50, 2 cameras)"""
    from syn3r_amd import measure
    from syn3r_amd.gs import OptimizationParams
    tr = measure.synthetic_scene(dev, TL.N, TL.H, TL.W, TL.VIEWS, 10, None)
    tr.opt = OptimizationParams(iterations=10, **fields)
    tr.reset_optimizers()
    return tr, tr.scene.getTrainCameras()


def _params(tr):
    return [p.detach().clone() for p in tr.gaussians.parameters()]


MCMC = dict(mcmc=True, densify_from_iter=0, mcmc_interval=2, mcmc_until_iter=1000)


@pytest.mark.parametrize("explicit", [True, False], ids=["explicit", "autograd"])
def test_trainer_grows_to_the_cap_and_stays(explicit, gpu):
    from syn3r_amd.gs import mcmc as M
    cap = 340
    tr, cams = make_trainer(gpu, mcmc_cap_max=cap, **MCMC)
    tr.densify = True
    g = tr.gaussians
    with torch.no_grad():
        g._opacity[:25] = -9.0                                        # dead on arrival
    dead = M.dead_logit(0.005)
    n, sizes, expect = TL.N, [], []
    for k in range(12):
        before = _params(tr)
        tr.train_step(cams[k % 2], explicit=explicit)
        ran = (k + 1) % 2 == 0
        if ran:
            n = min(cap, int(1.05 * n))
            # after a control call no Gaussian is at or below mcmc_min_opacity, and the optimiser step was skipped: the features of
            # the rows that were alive (not a destination; neither a source's adjustment nor the noise touches features) keep their bits
            assert bool((g._opacity.detach() > dead).all())
            alive = before[2] > dead
            assert torch.equal(g._features.detach()[:alive.shape[0]][alive].view(torch.int32), before[1][alive].view(torch.int32))
        else:
            assert not torch.equal(g._features.detach(), before[1])  # (an ordinary step moves them)
        sizes.append(int(g._xyz.shape[0]))
        expect.append(n)
    assert sizes == expect and sizes[-1] == cap and expect[:6] == [300, 315, 315, 330, 330, 340], sizes
    assert tr.mcmc.calls == 6
    for p in tr.gaussians.parameters():
        assert p.shape[0] == cap and bool(torch.isfinite(p).all())
        st = tr.optimizer.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
    assert g.confidence.shape[0] == cap
    # at the cap a control call changes neither N nor any allocation
    ptrs = [p.data_ptr() for p in tr.gaussians.parameters()]
    objs = [id(p) for p in tr.gaussians.parameters()]
    tr.train_step(cams[0], explicit=explicit)
    tr.train_step(cams[1], explicit=explicit)
    assert tr.mcmc.calls == 7
    assert [p.data_ptr() for p in tr.gaussians.parameters()] == ptrs and [id(p) for p in tr.gaussians.parameters()] == objs


def test_training_loop_with_the_option(gpu):
    """`GSTrainer.training` (the asynchronous loop: pair capacities seeded per (N, H, W) and carried over when N changes) with the
    option on: the control runs at iterations 2, 4, 6 and 8, N reaches the cap and the loss is finite."""
    tr, cams = make_trainer(gpu, mcmc_cap_max=340, **MCMC)
    loss = tr.training(0, iterations=8)
    assert math.isfinite(loss) and tr.mcmc.calls == 4 and tr.iteration == 8
    assert int(tr.gaussians._xyz.shape[0]) == 340
    for p in tr.gaussians.parameters():
        assert bool(torch.isfinite(p).all())
    # with densification disabled the control does not run; the regularisers and the noise still do
    tr2, _ = make_trainer(gpu, mcmc_cap_max=340, **MCMC)
    start = tr2.gaussians._xyz.detach().clone()
    tr2.training(0, iterations=4, disable_densification=True)
    assert tr2.mcmc.calls == 0 and int(tr2.gaussians._xyz.shape[0]) == 300 and not torch.equal(tr2.gaussians._xyz.detach(), start)


def test_trainer_routes_agree_on_one_step(gpu):
    """The explicit route (`syn3r_mcmc_reg_step` after the rasteriser backward) and the autograd route (torch operators on
    get_opacity / get_scaling) on one step with the option on: loss and raw-parameter gradients to the tolerance
    tests/test_trainer_gpu.py holds the two routes to (1e-6 on the loss, 2e-5 of the largest entry)."""
    grads = {}
    for explicit in (False, True):
        tr, cams = make_trainer(gpu, mcmc_cap_max=1000, mcmc_opacity_reg=0.05, mcmc_scale_reg=0.5, **MCMC)
        loss, _ = tr._explicit_step(cams[1]) if explicit else tr._autograd_step(cams[1])
        grads[explicit] = [float(loss.detach())] + [p.grad.detach().clone() for p in tr.gaussians.parameters()]
    off, cams = make_trainer(gpu)
    loss_off, _ = off._explicit_step(cams[1])
    assert grads[True][0] > float(loss_off) + 1e-4                    # the regularisers are in the loss
    assert not torch.equal(grads[True][3], off.gaussians._opacity.grad) and not torch.equal(grads[True][4], off.gaussians._scaling.grad)
    assert abs(grads[True][0] - grads[False][0]) < 1e-6
    for a, b in zip(grads[True][1:], grads[False][1:]):
        assert a.shape == b.shape
        scale = float(b.abs().max()) + 1e-20
        assert float((a - b).abs().max()) <= 2e-5 * scale, (float((a - b).abs().max()), scale)


def test_trainer_noise_runs_every_step_and_zero_launches_nothing(gpu):
    from syn3r_amd import _lib as L
    counts = {}
    for name, fields in (("on", dict(mcmc_cap_max=1000, **MCMC)), ("zero", dict(mcmc_cap_max=1000, mcmc_noise_lr=0.0, **MCMC)), ("off", {})):
        tr, cams = make_trainer(gpu, **fields)
        tr.train_step(cams[0])
        with L.kernel_trace() as trace:
            tr.train_step(cams[1])                                    # (iteration 2: the control runs when the trainer densifies; not here)
            tr.train_step(cams[0])
            torch.cuda.synchronize()
        counts[name] = {k: int(c) for k, (c, _) in trace.result.items()}
    mc = lambda d: {k: v for k, v in d.items() if "mcmc" in k}
    assert mc(counts["on"]) == {"k_mcmc_noise": 2, "k_mcmc_reg_pass": 2, "k_mcmc_reg_finish": 2}
    assert mc(counts["zero"]) == {"k_mcmc_reg_pass": 2, "k_mcmc_reg_finish": 2}
    assert mc(counts["off"]) == {}
    assert {k for k in counts["on"] if "mcmc" not in k} == set(counts["off"])


def test_off_is_off(gpu):
    """The option absent from the options (defaults) and spelled out as off with every other mcmc field changed: a short run with the
    density control on gives the same parameters bit for bit, with the same launches.  Two steps: an optimiser step (Adam's first
    step is lr * sign(grad), so its bits do not feel the order of the rasteriser's float atomics, as in the other off-is-off tests of
    the suite), then a step on which clone / split / prune run and the optimiser step is skipped."""
    from syn3r_amd import _lib as L
    results = []
    for fields in ({}, dict(mcmc=False, mcmc_cap_max=1, mcmc_noise_lr=1.0, mcmc_opacity_reg=1.0, mcmc_scale_reg=1.0, mcmc_interval=1,
                            mcmc_until_iter=10 ** 6, mcmc_min_opacity=0.5)):
        tr, cams = make_trainer(gpu, densify_from_iter=0, densification_interval=2, densify_until_iter=1000, **fields)
        tr.densify = True
        with L.kernel_trace() as trace:
            for k in range(2):
                tr.train_step(cams[k % 2])
            torch.cuda.synchronize()
        results.append((_params(tr), {k: int(c) for k, (c, _) in trace.result.items()}))
        assert tr.mcmc.calls == 0
    (pa, la), (pb, lb) = results
    assert la == lb and not [k for k in la if "mcmc" in k]
    for a, b in zip(pa, pb):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
