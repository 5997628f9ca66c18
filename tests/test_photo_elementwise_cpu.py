"""The checks of tests/test_photo_elementwise_gpu.py without a GPU: an fp32 restatement of k_photo_fwd and k_photo_bwd (csrc/photo_loss.hip: tile geometry,
row runs, halo indexing, ascending taps; tests/photo_ref.py) meets checks 1 to 5 on every design, so the derived bounds can be met
by a faithful fp32 implementation before a GPU is asked; each of nine subtly wrong restatements fails the check named for it."""
import numpy as np
import pytest

import photo_ref as R

F32, F64 = np.float32, np.float64


def restate(case, vec=None, mutant=None):
    a, b, m, _ = case.data
    maps, partial = R.restate_forward(a, b, m, vec, mutant)
    parts = R.restate_final(partial, case.shape, case.lam)
    with np.errstate(invalid="ignore"):
        grad = R.restate_backward(a, b, maps, case.lam, case.up, m, vec, mutant=mutant)
    return maps, partial, parts, grad


def run_checks(case, out):
    """{check: worst err / tol, or the CheckFailed} for checks 1 to 4."""
    maps, partial, parts, grad = out
    ref = case.data[3]
    equal = case.family == "conditioning" and case.name.rsplit("-", 1)[0] in R.EQUAL
    res = {}
    for k, fn in ((1, lambda: R.check_forward_pixels(ref, maps)),
                  (2, lambda: R.check_forward_tiles(ref, partial, parts, case.lam, equal)),
                  (3, lambda: R.check_backward_isolated(ref, maps, grad, case.lam, case.up)),
                  (4, lambda: R.check_end_to_end(ref, grad, case.lam, case.up))):
        try:
            res[k] = fn()
        except R.CheckFailed as e:
            res[k] = e
    return res


def test_constants_follow_the_counts():
    assert (R.GAMMA, R.GAMMA_B, R.DEPTH) == (24, 29, 12)
    w = R.window32()
    assert w.dtype == F32 and w.shape == (11,) and abs(float(w.astype(F64).sum()) - 1.0) < 1e-7 and np.array_equal(w, w[::-1])


def test_designs_cover_what_they_claim():
    shapes = [c.shape for c in R.CASES if c.family == "geometry"]
    tiles = {s[0] * R.grid(s)[0] * R.grid(s)[1] for s in shapes}
    assert {1, 2, 3, 5, 7, 8, 9, 12, 15, 16, 17, 23} <= tiles
    assert {r % 8 for r in tiles} == set(range(8))
    assert {s[2] % 4 for s in shapes} == {0, 1, 2, 3}
    assert {1, 2, 3, 4, 8, 11, 12} <= {s[2] for s in shapes} and {1, 5, 11} <= {s[1] for s in shapes}
    assert {31, 32, 33, 63, 64, 65} <= {v for s in shapes for v in s[1:]}
    assert {s[0] for s in shapes} == {1, 3, 5}
    geo = [c for c in R.CASES if c.family == "geometry"]
    assert {c.lam for c in geo} == {0.0, 0.2, 1.0} and {c.up for c in geo} == {None, 1.5}
    assert {c.kind for c in geo} == {None, "random", "rectangle", "zeros"}
    assert max(int(np.prod(s)) for s in shapes) == 3 * 97 * 131
    a, b = R.sweep_images((3, 64, 63))
    assert a.dtype == F32 and (b < 0).any() and (b > 1).any()
    assert (R.make_map("zeros", 32, 33) == 0).any() and R.make_map("rectangle", 65, 65)[31:34, 31:34].all()
    for shape, _ in R.ALIGNMENT:
        assert shape[2] % 4 == 0
    assert [s[2] % 4 == 0 for s in R.CONDITIONING_SHAPES] == [True, False]
    assert all(R.grid(s) == (2, 2) for s in R.CONDITIONING_SHAPES)


@pytest.mark.parametrize("nblk", [1, 2, 7, 8, 9, 23, 300])
def test_photo_tile_examples(nblk):
    assert sorted(R.photo_tile(b, nblk) for b in range(nblk)) == list(range(nblk))


def test_photo_tile_is_a_bijection():
    for nblk in range(1, 301):
        t = sorted(R.photo_tile(b, nblk) for b in range(nblk))
        assert t == list(range(nblk)), nblk
        if nblk % 8 and nblk > 8:
            assert sorted(R.photo_tile(b, nblk, "M8") for b in range(nblk)) != t


def test_reference_maps_are_the_gradient_of_the_published_loss():
    """The analytic float64 maps, windowed, are float64 autograd's gradient: the reference is consistent with itself."""
    for name in ("geom-3x37x53-lam0.2-up1.5-random", "geom-1x65x65-lam0.2-up1.5-rectangle", "anticorrelated-1x37x45"):
        case = R.CASE[name]
        ref = case.data[3]
        g, slack = ref.grad_from_stored(ref.maps, case.lam, case.up)
        auto = ref.grad_autograd(case.lam, case.up)
        c_l1, c_ssim = R.coefficients(case.shape, case.lam)
        # the float64 evaluations differ by float64 roundings and by c_l1, c_ssim rounded to fp32 (2^-24 relative)
        assert np.abs(g - auto).max() <= 4 * R.U * np.abs(auto).max() + 1e-12


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_restatement_meets_every_check(case, measurements):
    out = restate(case)
    res = run_checks(case, out)
    measurements("photo_restatement", case=case.name, family=case.family,
                 **{"check%d" % k: (v if isinstance(v, float) else str(v)) for k, v in res.items()})
    for v in res.values():
        if isinstance(v, R.CheckFailed):
            raise v
    if case.shape[2] % 4 == 0:                 # check 5: the non-VEC instantiation on a VEC-shaped image leaves the same bits
        for got, want, what in zip(restate(case, vec=False), out, ("maps", "tile sums", "parts", "gradient")):
            R.check_bits(what, got, want)


def shift_runs(mutant=None, shifts=R.SHIFTS):
    runs = {}
    for canvas in R.CANVASES:
        for offset in [R.CANONICAL] + list(shifts):
            a, b = R.shift_images(canvas, offset)
            maps, _ = R.restate_forward(a, b, mutant=mutant)
            runs[(canvas, offset)] = (maps, R.restate_backward(a, b, maps, 0.2, 1.5, mutant=mutant))
    return runs


def test_restatement_meets_the_shift_design():
    R.check_shift(shift_runs())


def test_shift_region_masks():
    inside, ys, xs, ok_maps, ok_grad = R.shift_region((3, 80, 83), (0, 60))
    assert not inside[:5].any() and ok_maps[5:, :18].all() and not ok_maps[5:, 24:].any()      # the patch's last column fell off
    assert R.shift_region((3, 80, 84), (60, 59))[3].sum() == 25 * 30                             # only the surround is clipped
    assert R.far_field((3, 80, 84), (0, 0)).sum() == 80 * 84 - 25 * 29


# per mutant: designs that reach it, the check that must catch it, and checks the mutant cannot touch (they must still pass)
SEAMS, PARTIAL_MAP = "geom-3x64x63-lam0.2-up1.5-None", "geom-3x37x53-lam0.2-up1.5-random"
MUTANT_TABLE = {
    "M1": (SEAMS, 1, ()),            # forward seam: per pixel in the stored maps
    "M2": (SEAMS, 3, (1, 2)),        # backward seam: only the backward in isolation sees it against the stored maps
    "M3": (SEAMS, 1, ()),
    "M4": (PARTIAL_MAP, 1, ()),
    "M5": (SEAMS, 1, (3,)),          # a wrong map is stored; the backward windows it faithfully
    "M6": (SEAMS, 3, (1, 2)),
    "M7": (PARTIAL_MAP, 1, ()),
    "M8": (SEAMS, 1, ()),            # 12 tiles: slots and map elements of the tiles that lost their block keep the NaN pattern
    "M9": (PARTIAL_MAP, 2, (1,)),    # only the tile's L1 sum
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_caught(mutant, measurements):
    name, catching, untouched = MUTANT_TABLE[mutant]
    case = R.CASE[name]
    clean = restate(case)
    out = restate(case, mutant=mutant)
    res = run_checks(case, out)
    failed = sorted(k for k, v in res.items() if isinstance(v, R.CheckFailed))
    ref = case.data[3]
    old = R.old_criteria_pass(ref, out[2], out[3], case.lam, case.up)
    assert R.old_criteria_pass(ref, clean[2], clean[3], case.lam, case.up)
    print("%s on %s: fails checks %s; the old criteria %s it" % (mutant, name, failed, "pass" if old else "catch"))
    measurements("photo_mutant", mutant=mutant, case=name, failed_checks=failed, old_criteria_pass=old)
    assert isinstance(res[catching], R.CheckFailed), "%s passes check %d" % (mutant, catching)
    for k in untouched:
        assert not isinstance(res[k], R.CheckFailed), "%s fails check %d, which it does not touch: %s" % (mutant, k, res[k])


@pytest.mark.parametrize("mutant", ["M1", "M2", "M3"])
def test_seam_mutants_break_the_shift_design(mutant):
    """Check 5: a dropped tap or replicated padding changes bits when the patch moves across a tile border."""
    with pytest.raises(R.CheckFailed) as e:
        R.check_shift(shift_runs(mutant, [(3, 3), (20, 20)]))
    assert e.value.check == 5


def test_nothing_is_skipped():
    """A bound that is not finite, or a value that was never written, fails; it is not masked."""
    case = R.CASE["geom-1x5x8-lam0-upNone-None"]
    maps, partial, parts, grad = restate(case)
    ref = case.data[3]
    bad = maps.copy()
    bad[1, 0, 2, 3] = np.nan
    with pytest.raises(R.CheckFailed):
        R.check_forward_pixels(ref, bad)
    with pytest.raises(R.CheckFailed):
        R._worst(1, "x", np.zeros(3), np.zeros(3), np.array([1.0, np.inf, 1.0]))
    with pytest.raises(R.CheckFailed):
        R._worst(1, "x", np.array([0.0, 1e-9]), np.zeros(2), np.zeros(2))
    assert R._worst(1, "x", np.zeros(2), np.zeros(2), np.zeros(2)) == 0.0
    for c in R.CASES:                           # the reference alone stays finite on every design
        r = c.data[3]
        assert np.isfinite(r.map_bounds).all() and np.isfinite(r.maps).all() and np.isfinite(r.tile_slack).all(), c.name
