"""3DGS-MCMC density control (`OptimizationParams.mcmc`), the parts that need no GPU: Philox4x32-10 known answers, the statistics of
the reference's normals, the ABI declarations and host-side refusals, the option fields and launcher flags, the trainer's two
ValueErrors, the refusal of CPU tensors, and the relocation formula at ratio 1 (tests/mcmc_ref.py is the reference of the GPU tests)."""
import dataclasses
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import mcmc_ref as R  # noqa: E402
from test_trainer_state_cpu import _trainer  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = ("syn3r_mcmc_noise", "syn3r_mcmc_reg_step_workspace_bytes", "syn3r_mcmc_reg_step", "syn3r_mcmc_weights",
           "syn3r_mcmc_sample_workspace_bytes", "syn3r_mcmc_sample", "syn3r_mcmc_relocate")


def test_philox_known_answers():
    hexs = lambda ws: " ".join(f"{int(w):08x}" for w in ws)
    assert hexs(R.philox(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexs(R.philox(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # the counter layout: (index, 0, tag, step), key = (seed low, seed high); arrays and ints agree
    a = R.words(np.arange(5, dtype=np.uint64), R.TAG_SAMPLE, 7, (3 << 32) | 9)
    b = R.philox(4, 0, 1, 7, 9, 3)
    assert [int(w[4]) for w in a] == [int(w) for w in b]


def test_reference_normals_are_standard_normal():
    n = 65536
    eps, rad = R.normals(np.arange(n, dtype=np.uint64), step=3, seed=11)
    assert eps.shape == (n, 3) and bool(np.isfinite(eps).all()) and bool((np.abs(eps) <= rad * (1 + 1e-12)).all())
    se_mean, se_var, se_corr = 1.0 / math.sqrt(n), math.sqrt(2.0 / n), 1.0 / math.sqrt(n)
    assert float(np.abs(eps.mean(axis=0)).max()) <= 5 * se_mean
    assert float(np.abs(eps.var(axis=0) - 1.0).max()) <= 5 * se_var
    c = np.corrcoef(eps.T)
    assert float(np.abs(c - np.eye(3)).max()) <= 5 * se_corr
    # another step, another seed: other draws
    assert not np.array_equal(eps, R.normals(np.arange(n, dtype=np.uint64), step=4, seed=11)[0])
    assert not np.array_equal(eps, R.normals(np.arange(n, dtype=np.uint64), step=3, seed=12)[0])


def test_header_declares_the_entries_and_the_binding_has_them():
    from syn3r_amd import _lib as L
    from syn3r_amd import build as B
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "syn3r_hip.h").read_text(), flags=re.S)
    lib = L.load()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert L.SIGNATURES["syn3r_mcmc_noise"] == (L.c_i, [L.c_p, L.c_p, L.c_p, L.c_p, L.c_i, L.c_f, L.c_ll, L.c_i, L.c_p])
    assert L.SIGNATURES["syn3r_mcmc_sample"] == (L.c_i, [L.c_p, L.c_i, L.c_i, L.c_ll, L.c_i, L.c_p, L.c_p, L.c_p, L.c_sz, L.c_p])
    assert "mcmc.hip" in B.STRICT_FP


def test_entries_reject_bad_arguments_before_any_launch():
    """null pointers, n = 0 and 2^24 + 1, a short workspace, aliasing, misalignment: a status and a message"""
    import ctypes as C
    from syn3r_amd import _lib as L
    lib = L.load()
    buf = (C.c_float * 16384)()
    base = (C.addressof(buf) + 255) & ~255
    a, b, c, d, e, f, g, ws = (base + 4096 * k for k in range(8))
    err = lambda: lib.syn3r_last_error().decode()
    big = 2 ** 24 + 1
    # noise
    assert lib.syn3r_mcmc_noise(None, b, c, d, 4, 1.0, 0, 0, None) == -1 and "null" in err()
    assert lib.syn3r_mcmc_noise(a, b, c, d, 0, 1.0, 0, 0, None) == -1 and lib.syn3r_mcmc_noise(a, b, c, d, big, 1.0, 0, 0, None) == -1
    assert lib.syn3r_mcmc_noise(a, a + 8, c, d, 4, 1.0, 0, 0, None) == -1 and "alias" in err()
    assert lib.syn3r_mcmc_noise(a, b, c + 4, d, 4, 1.0, 0, 0, None) == -1 and "align" in err()
    assert lib.syn3r_mcmc_noise(a, b, c, d, 4, float("nan"), 0, 0, None) == -1
    # regularisers
    assert lib.syn3r_mcmc_reg_step_workspace_bytes(0) == 0 == lib.syn3r_mcmc_reg_step_workspace_bytes(big)
    need = lib.syn3r_mcmc_reg_step_workspace_bytes(4)
    assert need >= 8 and need % 256 == 0 and lib.syn3r_mcmc_reg_step_workspace_bytes(2 ** 24) == 2048 * 2 * 4
    assert lib.syn3r_mcmc_reg_step(a, b, 4, 0.01, 0.01, c, d, None, ws, need, None) == -1 and "null" in err()
    assert lib.syn3r_mcmc_reg_step(a, b, 0, 0.01, 0.01, c, d, e, ws, need, None) == -1
    assert lib.syn3r_mcmc_reg_step(a, b, big, 0.01, 0.01, c, d, e, ws, need, None) == -1
    assert lib.syn3r_mcmc_reg_step(a, b, 4, 0.01, 0.01, c, d, e, ws, need - 1, None) == -2 and "workspace" in err()
    assert lib.syn3r_mcmc_reg_step(a, b, 4, 0.01, 0.01, a, d, e, ws, need, None) == -1 and "alias" in err()
    assert lib.syn3r_mcmc_reg_step(a, b, 4, 0.01, 0.01, c, c + 8, e, ws, need, None) == -1 and "alias" in err()
    # weights
    assert lib.syn3r_mcmc_weights(a, 4, -5.0, None, None) == -1 and "null" in err()
    assert lib.syn3r_mcmc_weights(a, 0, -5.0, b, None) == -1 and lib.syn3r_mcmc_weights(a, big, -5.0, b, None) == -1
    assert lib.syn3r_mcmc_weights(a, 4, -5.0, a + 4, None) == -1 and "alias" in err()
    # sampling
    assert lib.syn3r_mcmc_sample_workspace_bytes(0) == 0 == lib.syn3r_mcmc_sample_workspace_bytes(big)
    need = lib.syn3r_mcmc_sample_workspace_bytes(4)
    assert need >= 4 * 4 + 4 + 16 and lib.syn3r_mcmc_sample_workspace_bytes(70000) >= 70000 * 4 + 18 * 4 + 19 * 8
    assert lib.syn3r_mcmc_sample(a, 4, 0, 0, 0, None, c, ws, need, None) == -1 and "null" in err()
    assert lib.syn3r_mcmc_sample(a, 0, 0, 0, 0, b, c, ws, need, None) == -1 and lib.syn3r_mcmc_sample(a, big, 0, 0, 0, b, c, ws, need, None) == -1
    assert lib.syn3r_mcmc_sample(a, 4, -1, 0, 0, b, c, ws, need, None) == -1 and "m_extra" in err()
    assert lib.syn3r_mcmc_sample(a, 4, 0, 0, 0, b, c, ws, need - 1, None) == -2 and "workspace" in err()
    assert lib.syn3r_mcmc_sample(a, 4, 2, 0, 0, b, b + 20, ws, need, None) == -1 and "alias" in err()
    # relocation
    mom = (C.c_void_p * 10)()
    assert lib.syn3r_mcmc_relocate(4, a, b, c, d, 12, e, f, None, mom, 0.005, None) == -1 and "null" in err()
    assert lib.syn3r_mcmc_relocate(4, a, b, c, d, 12, e, f, g, None, 0.005, None) == -1 and "null" in err()
    assert lib.syn3r_mcmc_relocate(0, a, b, c, d, 12, e, f, g, mom, 0.005, None) == -1
    assert lib.syn3r_mcmc_relocate(big, a, b, c, d, 12, e, f, g, mom, 0.005, None) == -1
    assert lib.syn3r_mcmc_relocate(4, a, b, c, d, 0, e, f, g, mom, 0.005, None) == -1 and "feature_row_len" in err()
    assert lib.syn3r_mcmc_relocate(4, a, b, c, c + 16, 12, e, f, g, mom, 0.005, None) == -1 and "alias" in err()
    assert lib.syn3r_mcmc_relocate(4, a, b, c, d, 12, e, f, g, mom, 0.0, None) == -1 and "min_opacity" in err()


def test_fields_defaults_and_launcher_flags():
    from syn3r_amd import launch
    from syn3r_amd.gs import OptimizationParams
    d = OptimizationParams()
    assert (d.mcmc, d.mcmc_cap_max, d.mcmc_noise_lr, d.mcmc_opacity_reg, d.mcmc_scale_reg, d.mcmc_interval, d.mcmc_until_iter,
            d.mcmc_min_opacity) == (False, 200_000, 5e5, 0.01, 0.01, 100, 25_000, 0.005)
    base = OptimizationParams(iterations=77, lambda_dssim=0.3, seed=4)
    assert launch.apply_trainer_flags(base, launch.parse(["--scenes", "x"])) == base
    assert launch.apply_trainer_flags(base, launch.parse(["--scenes", "x", "--mcmc", "0"])) == base
    on = launch.apply_trainer_flags(base, launch.parse(["--scenes", "x", "--mcmc", "1"]))
    changed = {f.name for f in dataclasses.fields(base) if getattr(on, f.name) != getattr(base, f.name)}
    assert changed == {"mcmc"} and on.mcmc is True
    full = launch.apply_trainer_flags(base, launch.parse(["--scenes", "x", "--mcmc=1", "--mcmc_cap_max", "5000", "--mcmc_noise_lr", "1e4",
                                                           "--mcmc_opacity_reg", "0.02", "--mcmc_scale_reg", "0.03"]))
    assert (full.mcmc, full.mcmc_cap_max, full.mcmc_noise_lr, full.mcmc_opacity_reg, full.mcmc_scale_reg, full.mcmc_interval) == \
        (True, 5000, 1e4, 0.02, 0.03, 100)
    for bad in (["--mcmc", "2"], ["--mcmc_cap", "5"], ["--mcm", "1"], ["--mcmc_noise", "1.0"], ["--mcmc_scale", "0.1"]):
        with pytest.raises(SystemExit):
            launch.parse(["--scenes", "x"] + bad)


def test_trainer_refuses_contradictory_options():
    with pytest.raises(ValueError, match="use_proximity_densify"):
        _trainer(mcmc=True, use_proximity_densify=True)
    with pytest.raises(ValueError, match="densify_abs_grad"):
        _trainer(mcmc=True, densify_abs_grad=True)
    with pytest.raises(ValueError, match="mcmc_cap_max"):
        _trainer(n=6, mcmc=True, mcmc_cap_max=5)
    tr, _ = _trainer(n=6, mcmc=True, mcmc_cap_max=6)
    assert tr.mcmc.calls == 0
    _trainer(use_proximity_densify=True, densify_abs_grad=True, mcmc_cap_max=1)      # option off: the fields are not looked at


def test_cpu_tensors_are_refused():
    from syn3r_amd import _lib as L
    from syn3r_amd.gs import train_ops as T
    n = 5
    xyz, ls, rot, lg, feat = torch.zeros(n, 3), torch.zeros(n, 3), torch.ones(n, 4), torch.zeros(n), torch.zeros(n, 4, 3)
    with pytest.raises(L.Syn3rError):
        T.mcmc_noise(xyz, ls, rot, lg, 1.0, 0, 0)
    with pytest.raises(L.Syn3rError):
        T.mcmc_reg_step(lg, ls, 0.01, 0.01, torch.zeros(n), torch.zeros(n, 3))
    with pytest.raises(L.Syn3rError):
        T.mcmc_weights(lg, -5.0)
    with pytest.raises(L.Syn3rError):
        T.mcmc_sample(torch.ones(n, dtype=torch.int32), 0, 0, 0)
    with pytest.raises(L.Syn3rError):
        T.mcmc_relocate(torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), xyz, feat, lg, ls, rot, [None] * 10, 0.005)
    tr, _ = _trainer(mcmc=True, mcmc_cap_max=10)
    with pytest.raises(L.Syn3rError):
        tr.mcmc.relocate_and_grow(100)


def test_control_schedule_and_clamp():
    from syn3r_amd.gs import mcmc as M
    tr, _ = _trainer(mcmc=True, mcmc_cap_max=10, densify_from_iter=100, mcmc_interval=50, mcmc_until_iter=300)
    ran = []
    tr.mcmc.relocate_and_grow = lambda step: ran.append(step)
    for it in range(400):
        tr.iteration = it
        tr.mcmc.control({})
    assert ran == [150, 200, 250] and tr.mcmc.calls == 3
    # the lower clamp of a relocated opacity: at or a hair above the threshold, and alive under the dead test
    for m in (0.005, 0.01, 0.001):
        dead, c = np.float32(M.dead_logit(m)), M.clamp_opacity(m)
        assert m <= c <= m * (1 + 1e-5) and c == float(np.float32(c))
        assert np.float32(math.log(c / (1.0 - c))) > dead


def test_relocation_reference_sanity():
    # ratio 1 (never drawn): opacity and scale unchanged
    for o in (0.005, 0.1, 0.5, 0.9, 0.999999):
        on, f, cond = R.relocation(o, 0, 0.005)
        assert abs(on - o) <= 1e-15 and abs(f - 1.0) <= 1e-14 and abs(cond - 1.0) <= 1e-14
    # the double sum collapses to sum_m C(ratio, m) (-1)^(m-1) o'^m / sqrt(m) (what the kernel evaluates)
    for o, c in ((0.5, 2), (0.9, 9), (0.99, 50), (0.1, 200)):
        on, f, cond = R.relocation(o, c, 0.005)
        ratio = min(c + 1, 51)
        D = math.fsum(math.comb(ratio, m) * (-1.0) ** (m - 1) * on ** m / math.sqrt(m) for m in range(1, ratio + 1))
        assert abs(o / D - f) <= 1e-9 * cond * abs(f)
        assert 0.0 < on < o and (on == 0.005 or abs((1 - on) ** ratio - (1 - o)) <= 1e-12)      # (0.1, 200: the lower clamp)
    # the cancellation the issue quotes
    assert 8.0e3 < R.relocation(0.999999, 50, 0.005)[2] < 1.0e4 and R.relocation(0.99, 50, 0.005)[2] <= 24.0
    # integer sampling: zero weights are never drawn, counts add up
    w = [0, 5, 0, 0, 3, 0, 1, 0]
    src, counts = R.sample(w, 3, seed=1, step=2)
    assert src.shape == (11,) and all(src[d] == -1 for d in (1, 4, 6)) and all(w[int(s)] > 0 for s in src if s >= 0)
    assert int(counts.sum()) == 8 and np.array_equal(counts, np.bincount(src[src >= 0], minlength=8))
    assert bool((R.sample([0, 0, 0], 2, 1, 2)[0] == -1).all())
