"""What tests/raster_proj_ref.py says about its scenes, checked on the float64 reference, and the proof that the per-Gaussian measure
with the committed bars catches each of the twelve mutants - without a GPU, in seconds.  tests/test_raster_proj_gpu.py holds the
kernels to the same references."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_proj_ref as P  # noqa: E402
from oracle import raster_oracle as RO  # noqa: E402

LOSSES = ("full", "colour")


def denominators(ref, conf=True):
    """{group: the smallest per-Gaussian denominator over the visible Gaussians}"""
    groups = [g for g in P.GROUPS if conf or g != "cf"]
    return {g: float(P.per_gaussian(g, ref["grads"][g], ref["grads"][g])[1][ref["valid"]].min()) for g in groups}


# ------------------------------------------------------------------------------------------------------------------ scenes
@pytest.mark.parametrize("mode", list(P.MODES))
def test_lattice(mode):
    """all 20 present and isolated, no radius on an edge, every denominator well above zero (>= 0.9 under the full loss without the 3D
    filter; >= 0.01 with it, whose coef takes the gradients down with the opacity, and under the colour-only loss, where colour minus
    background changes sign between the channels); the two Gaussians with a zero filter are there"""
    sc = P.lattice()
    assert int((sc["f"] == 0).sum()) == 2 and float(sc["f"][sc["f"] > 0].min() / sc["s"].mean(1).max()) > 0.05
    for loss in LOSSES:
        for conf in (True, False):
            ref = P.reference(sc, 3, mode, loss, conf=conf)
            assert int(ref["valid"].sum()) == 20 and P.isolated(ref) and P.radius_edges(ref) == 0
            assert int(ref["px_alpha"].sum((1, 2)).min()) >= 30
            den = denominators(ref, conf)
            print(mode, loss, conf, "largest radius", int(ref["radius"].max()), {k: f"{v:.3g}" for k, v in den.items()})
            assert min(den.values()) >= (0.01 if P.MODES[mode][1] or loss == "colour" else 0.9), den
    if mode == "plain":
        assert int(ref["radius"].max()) == 10


@pytest.mark.parametrize("mode", list(P.MODES))
def test_guard(mode):
    """every guard Gaussian is visible with every gradient group non-zero; from the reference's view-space means: two beyond the band
    in x (both signs) and two in y (both signs), the corner one beyond it in both, the controls inside it"""
    beyond_x, beyond_y = [], []
    for which in P.GUARD:
        sc = P.guard(which)
        for loss in LOSSES:
            ref = P.reference(sc, 3, mode, loss)
            assert bool(ref["valid"][0]) and P.radius_edges(ref) == 0 and int(ref["px_alpha"].sum()) >= 20
            den = denominators(ref)
            assert min(den.values()) > 0.05, (which, den)
        t = ref["t"][0]
        ax, ay = float(t[0] / t[2]) / (1.3 * sc["tfx"]), float(t[1] / t[2]) / (1.3 * sc["tfy"])
        if abs(ax) > 1:
            beyond_x.append(np.sign(ax))
        if abs(ay) > 1:
            beyond_y.append(np.sign(ay))
        if which == "corner":
            assert abs(ax) > 1 and abs(ay) > 1
        if which.startswith("ctl"):
            assert 0.95 < max(abs(ax), abs(ay)) < 1
        if mode == "plain" and loss == "colour":
            print(which, "radius", int(ref["radius"][0]), "pixels", int(ref["px_alpha"].sum()), {k: f"{v:.3g}" for k, v in den.items()})
    assert sorted(beyond_x) == [-1, 1, 1] and sorted(beyond_y) == [-1, 1, 1]          # x+, x-, corner / y+, y-, corner


def test_clamp():
    """the clamp mask takes each value 0 .. 7, no channel's colour before the clamp within 1e-3 of 0; the only zero denominator of
    any scene is the SH gradient of the Gaussian whose three channels are clamped"""
    sc = P.clamp_scene()
    dirs = sc["m"] - sc["campos"][None]
    raw = RO.eval_sh(3, sc["sh"], dirs / dirs.norm(dim=1, keepdim=True)) + 0.5
    assert float(raw.abs().min()) >= 1e-3
    for loss in LOSSES:
        ref = P.reference(sc, 3, "plain", loss)
        assert ref["clamped"].tolist() == list(range(8)) and bool(ref["valid"].all()) and P.isolated(ref) and P.radius_edges(ref) == 0
        for g in P.GROUPS:
            den = P.per_gaussian(g, ref["grads"][g], ref["grads"][g])[1]
            assert bool((den[:7] > 0).all()), g
            assert (float(den[7]) == 0.0) == (g == "sh"), g
        gsh = ref["grads"]["sh"]
        for k in range(8):
            for c in range(3):
                assert (float(gsh[k, :, c].abs().max()) == 0.0) == bool((k >> c) & 1)


@pytest.mark.parametrize("N", P.BLOCK_N)
def test_blocks(N):
    sc = P.blocks(N)
    ref = P.reference(sc, 3, "plain", "full")
    assert torch.nonzero(ref["valid"]).reshape(-1).tolist() == sc["slots"] and P.radius_edges(ref) == 0
    assert [k == "visible" for k in sc["kind"]] == ref["valid"].tolist()
    if N > 8:
        assert all(sc["kind"].count(k) >= (N - 8) // 4 for k in P.CULL_KINDS)
    t = ref["t"]
    for i, k in enumerate(sc["kind"]):          # each kind is culled for ITS reason
        if k == "behind":
            assert float(t[i, 2]) < 0
        elif k == "near":
            assert 0 < float(t[i, 2]) < 0.2
        elif k in ("off_axis", "off_edge"):
            assert float(t[i, 2]) > 0.2 and int(ref["tiles_touched"][i]) == 0
            assert (abs(float(t[i, 0] / t[i, 2])) < 1.3 * sc["tfx"]) == (k == "off_edge")
    den = denominators(ref)
    assert min(den.values()) > 0.9, den


def test_near():
    """the float32 t.z of every Gaussian lies on the intended side of 0.2f (the view matrix is the identity: the kernel's t.z is the
    mean's z exactly), Gaussian 8 exactly ON it; the far ones are visible, point-like, with non-zero denominators"""
    sc = P.near_scene()
    assert torch.equal(sc["view"], torch.eye(4, dtype=torch.float64))
    v, m = sc["view"].float(), sc["m"].float()
    tz = v[0, 2] * m[:, 0] + v[1, 2] * m[:, 1] + v[2, 2] * m[:, 2] + v[3, 2]          # xf43's expression, in float32
    near = torch.tensor(0.2, dtype=torch.float32)
    assert bool((tz[0:8:2] < near).all()) and bool((tz[1:8:2] > near).all()) and bool(tz[8] == near)
    assert float(tz[1:8:2].max()) < 0.2 * (1 + 2 * P.NEAR_EPS) and float(tz[0:8:2].min()) > 0.2 * (1 - 2 * P.NEAR_EPS)
    for loss in LOSSES:
        ref = P.reference(sc, 3, "plain", loss)
        assert ref["valid"].tolist() == [False, True] * 4 + [False]
        assert P.isolated(ref) and P.radius_edges(ref) == 0 and ref["radius"][ref["valid"]].tolist() == [3] * 4
        den = denominators(ref)
        print(loss, {k: f"{v:.3g}" for k, v in den.items()})
        assert min(den.values()) > 0, den


@pytest.mark.parametrize("sm", [0.5, 2.0])
@pytest.mark.parametrize("mode", list(P.MODES))
def test_scale_modifier_scenes_keep_the_footprints(sm, mode):
    lat = P.lattice()
    base, ref = P.reference(lat, 3, mode), P.reference(P.with_modifier(lat, sm), 3, mode, sm=sm)
    assert torch.equal(base["radius"], ref["radius"]) and torch.equal(base["tiles_touched"], ref["tiles_touched"])
    assert P.isolated(ref) and P.radius_edges(ref) == 0 and bool(ref["valid"].all())
    assert float((ref["conic"] - base["conic"]).abs().max() / base["conic"].abs().max()) < 1e-6          # the scales' rounding alone
    den = denominators(ref)
    assert min(den.values()) > 0.02, den


@pytest.mark.parametrize("deg,M", P.SH_LAYOUTS)
def test_sh_layout_scenes(deg, M):
    ref = P.reference(P.with_coeffs(P.lattice(), M), deg)
    assert bool(ref["valid"].all()) and min(denominators(ref).values()) > 0.1
    gsh = ref["grads"]["sh"]
    assert gsh.shape[1] == M and float(gsh[:, (deg + 1) ** 2:].abs().sum()) == 0.0
    assert bool((gsh[:, :(deg + 1) ** 2].abs().amax(dim=(0, 2)) > 0).all())


def test_raw_route_scenes():
    """the raw references: activations in float64 of the float32 parameters, chain rule in float64; denominators above zero at every
    quaternion norm"""
    lat = P.lattice()
    for k in (None,) + P.RAW_NORMS:
        raw = P.raw_params(lat, k)
        ref = P.reference(lat, 3, "f3d_aa", raw=raw, tag=k)
        assert bool(ref["valid"].all()) and P.isolated(ref) and P.radius_edges(ref) == 0
        for g in ("s", "q", "o"):
            den = P.per_gaussian(g, ref["grads_raw"][g], ref["grads_raw"][g])[1]
            assert float(den.min()) > 0, (k, g)
        if k is not None:
            np.testing.assert_allclose(raw["q"].norm(dim=1).numpy(), k, rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------------ mutants
def test_every_patch_applies_and_the_unpatched_reference_is_the_oracle():
    for mutant in P.MUTANTS:
        assert P.patched_preprocess(mutant) is not None
    assert P.patched_preprocess(None) is RO.preprocess
    assert len(P.MUTANTS) == 12 and len(set(P.MUTANTS)) == 12


def test_backward_conic_formulas_are_the_oracles_derivative():
    """the restated formulas of k_preprocess_bwd (dL_dA / dL_dB / dL_dC with den2inv) under the oracle give the oracle's own
    gradients up to the regulariser 1e-7 / den^2 (den >= 1.6 on the lattice): the `lowpass_not_in_den` mutant differs from the
    reference in `den` alone"""
    lat = P.lattice()
    ref, alt = P.reference(lat, 3, "aa"), P.reference(lat, 3, "aa", mutant="_conic_formulas")
    for g in P.GROUPS:
        rel, _ = P.per_gaussian(g, alt["grads"][g], ref["grads"][g])
        assert float(rel.max()) < 1e-7, (g, float(rel.max()))


def _mutant_cases():
    """mutant -> (what to compare, reference arguments, group): the scene built for it"""
    lat = P.lattice()
    return {
        "guard_mul_omitted": (P.guard("x+"), dict(), "m"),
        "guard_limit_1": (P.guard("ctl_x"), dict(), "m"),
        "clamp_ignored": (P.clamp_scene(), dict(), "sh"),
        "clamp_rotated": (P.clamp_scene(), dict(), "sh"),
        "modifier_not_in_dscale": (P.with_modifier(lat, 2.0), dict(sm=2.0), "s"),
        "modifier_in_coef": (P.with_modifier(lat, 2.0), dict(sm=2.0, mode="f3d"), "o"),
        "sh3_term_dropped": (lat, dict(), "m"),
        "dsigma_offdiag_not_doubled": (lat, dict(), "s"),
        "raw_quat_not_projected": (lat, dict(raw=P.raw_params(lat), tag=None), "q"),
        "conf_not_in_dopacity": (lat, dict(), "o"),
        "lowpass_not_in_den": (lat, dict(), "s"),
    }


@pytest.mark.parametrize("mutant", [m for m in P.MUTANTS if m != "near_lt"])
def test_mutant_is_caught_by_the_per_gaussian_measure(mutant):
    """the mutant moves at least one Gaussian of its scene by >= 10 x the committed bar of its group (most move every one)"""
    sc, kw, group = _mutant_cases()[mutant]
    ref, mut = P.reference(sc, 3, **kw), P.reference(sc, 3, mutant=mutant, **kw)
    which = "grads_raw" if kw.get("raw") is not None else "grads"
    rel, _ = P.per_gaussian(group, mut[which][group], ref[which][group])
    rel = rel[ref["valid"]]
    bar = P.BAR["guard" if mutant.startswith("guard") else "lattice"]["q_raw" if which == "grads_raw" and group == "q" else group]
    print(f"{mutant}: group {group}: per-Gaussian rel min {float(rel.min()):.3g} max {float(rel.max()):.3g}; bar {bar:.1e}; "
          f"Gaussians over 10 x bar: {int((rel >= 10 * bar).sum())} of {rel.numel()}")
    assert float(rel.max()) >= 10 * bar


def test_mutant_near_lt_is_caught_by_the_culled_set():
    """`t.z < kNearClip` keeps the Gaussian AT float32(0.2): the forward check's exact culled set sees it"""
    sc = P.near_scene()
    ref, mut = P.reference(sc, 3), P.reference(sc, 3, mutant="near_lt")
    assert not bool(ref["valid"][8]) and bool(mut["valid"][8]) and int(mut["radius"][8]) > 0
    assert torch.equal(ref["valid"][:8], mut["valid"][:8])


GLOBAL_BAR = 2e-3          # tests/test_raster_gpu.py::test_backward_vs_autograd and the mode files


# mutant -> does the one-bar-per-tensor measure let it through on the mixed scene?
GLOBAL_BLIND = {"guard_mul_omitted": False, "clamp_ignored": False, "sh3_term_dropped": True}


@pytest.mark.parametrize("mutant", list(GLOBAL_BLIND))
def test_global_measure_on_a_mixed_scene(mutant):
    """A scene like the older tests' (a random mid-frustum field) to which the edge-case Gaussians were ADDED.  The per-Gaussian
    measure is far over its bar for all three mutants.  The one-bar-per-tensor measure (< 2e-3) lets `sh3_term_dropped` through:
    7.3e-4 of the largest dL/dmean, where single Gaussians are off by 0.66 % of their own.  It does NOT let the other two through, as
    had been supposed: a guard-band Gaussian of this size moves dL/dmean by 0.066 of the tensor's largest entry and the eight
    clamped ones dL/dsh by 0.4 - what kept those two branches unseen was that no scene REACHED them, not the measure.  The mutants
    stay."""
    sc = P.mixed_scene()
    ref, mut = P.reference(sc, 3), P.reference(sc, 3, mutant=mutant)
    worst_global = max(P.global_measure(mut["grads"][g], ref["grads"][g]) for g in P.GROUPS)
    worst_local = max(float(P.per_gaussian(g, mut["grads"][g], ref["grads"][g])[0][ref["valid"]].max()) for g in P.GROUPS)
    print(f"{mutant}: global measure {worst_global:.3g}, worst per-Gaussian {worst_local:.3g}")
    assert worst_local >= 10 * max(max(P.BAR[f].values()) for f in ("lattice", "guard"))
    assert (worst_global < GLOBAL_BAR) == GLOBAL_BLIND[mutant]
