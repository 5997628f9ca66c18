"""Anti-aliased splatting (the published `antialiasing` switch: Mip-Splatting's 2D Mip filter) without a GPU: the gradient formulas
the backward kernel restates, the settings field, the launcher flag, and the energy property on the float64 reference
(tests/raster_aa_ref.py) alone."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_aa_ref as R  # noqa: E402

H_LP, FLOOR = 0.3, 0.000025


def _formulas(a, b, c, dL_drho):
    """include/syn3r_hip.h, SYN3R_RASTER_ANTIALIAS: -> (rho, dL/da, dL/db, dL/dc) in the dtype of the inputs"""
    A, C = a + H_LP, c + H_LP
    d0, d1 = a * c - b * b, A * C - b * b
    r = d0 / d1
    rho = torch.sqrt(torch.clamp(r, min=FLOOR))
    dL_dr = torch.where(r > FLOOR, dL_drho / (2.0 * rho), torch.zeros_like(r))
    dr_da = (c * d1 - C * d0) / (d1 * d1)
    dr_dc = (a * d1 - A * d0) / (d1 * d1)
    dr_db = -2.0 * b * (d1 - d0) / (d1 * d1)
    return rho, dL_dr * dr_da, dL_dr * dr_db, dL_dr * dr_dc


def _kernel_forms(a, b, c):
    """the cancellation-free right-hand sides k_preprocess_bwd evaluates (csrc/raster_bwd.hip): h taken out of the numerators"""
    A, C = a + H_LP, c + H_LP
    d1 = A * C - b * b
    return H_LP * (c * C + b * b) / (d1 * d1), -2.0 * b * H_LP * (a + C) / (d1 * d1), H_LP * (a * A + b * b) / (d1 * d1)


def test_gradient_formulas_equal_autograd():
    g = torch.Generator().manual_seed(11)
    n = 4096
    # covariances L L^T over six decades of size: d0 > 0
    l00 = torch.exp(torch.empty(n, dtype=torch.float64).uniform_(-4.0, 4.0, generator=g))
    l11 = torch.exp(torch.empty(n, dtype=torch.float64).uniform_(-4.0, 4.0, generator=g))
    l10 = torch.randn(n, generator=g, dtype=torch.float64) * l00
    a, b, c = l00 * l00, l00 * l10, l10 * l10 + l11 * l11
    w = torch.randn(n, generator=g, dtype=torch.float64)
    leaves = [t.clone().requires_grad_(True) for t in (a, b, c)]
    A, C = leaves[0] + H_LP, leaves[2] + H_LP
    r = (leaves[0] * leaves[2] - leaves[1] ** 2) / (A * C - leaves[1] ** 2)
    rd = r.detach()
    assert float(rd.min()) > 0 and int((rd > FLOOR).sum()) > n // 2 and int((rd < FLOOR).sum()) > 0
    (torch.sqrt(torch.clamp(r, min=FLOOR)) * w).sum().backward()
    rho, da, db, dc = _formulas(a, b, c, w)
    above = r.detach() > FLOOR
    for got, leaf in zip((da, db, dc), leaves):
        ref = leaf.grad
        err = ((got - ref).abs() / ref.abs().clamp(min=1e-300))[above]
        assert float(err.max()) < 1e-10, float(err.max())
        assert (got[~above] == 0).all() and (ref[~above] == 0).all()       # under the floor: exactly no gradient
    # and the forms the kernel evaluates are the same polynomials
    Ad, Cd = a + H_LP, c + H_LP
    d0, d1 = a * c - b * b, Ad * Cd - b * b
    issue_forms = ((c * d1 - Cd * d0) / d1 ** 2, -2.0 * b * (d1 - d0) / d1 ** 2, (a * d1 - Ad * d0) / d1 ** 2)
    for got, ref in zip(_kernel_forms(a, b, c), issue_forms):
        assert float(((got - ref).abs() / ref.abs().clamp(min=1e-300)).max()) < 1e-9


def test_settings_field_is_last_and_off():
    from syn3r_amd.raster import GaussianRasterizationSettings
    assert GaussianRasterizationSettings._fields[-1] == "antialiasing"
    assert GaussianRasterizationSettings._field_defaults["antialiasing"] is False
    z = torch.zeros(3)
    st = GaussianRasterizationSettings(4, 4, 1.0, 1.0, z, 1.0, z, z, 0, z, False, True)      # positional callers are unaffected
    assert st.debug is True and st.antialiasing is False


def test_launcher_flag_reaches_optimization_params():
    from syn3r_amd import launch
    from syn3r_amd.gs import OptimizationParams
    assert OptimizationParams().antialiasing is False
    on = launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "a", "--antialiasing", "1"]))
    assert on.antialiasing is True
    off = launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "a"]))
    assert off.antialiasing is False
    off = launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "a", "--antialiasing", "0"]))
    assert off.antialiasing is False
    with pytest.raises(SystemExit):
        launch.parse(["--scenes", "a", "--antialias", "1"])


@pytest.mark.parametrize("z", [2.0, 4.0])
def test_reference_keeps_the_energy_of_a_small_splat(z):
    """One isotropic Gaussian: sum(alpha) over its true footprint op 2 pi sigma_px^2.  Measured on the reference: 0.991 and 0.967
    with the filter, 1.97 and 4.89 without (z = 8 is left out on purpose: there the 1/255 alpha cut-off removes 12 %)."""
    sc = R.single_gaussian(z)
    with torch.no_grad():
        (_, _, _, a_on, _), _, _, _ = R.rasterize(sc, 0, True)
        (_, _, _, a_off, _), _, _, _ = R.rasterize(sc, 0, False)
    fp = R.footprint(sc, z)
    on, off = float(a_on.sum()) / fp, float(a_off.sum()) / fp
    print(f"z = {z}: sum(alpha) / footprint = {on:.4f} with the filter, {off:.4f} without")
    assert 0.95 <= on <= 1.01, on
    assert off >= 1.9, off
