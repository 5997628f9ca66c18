"""AbsGS' absolute screen-space gradient without a GPU: the float64 reference of tests/raster_absgrad_ref.py is pinned to the oracle,
its scenes exercise what the blend backward can get wrong (several staging rounds, the early stop, exact cancellation of the plain
sum), and the host plumbing (header, ctypes table, launcher flags, OptimizationParams) is in place."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import raster_aa_ref as A  # noqa: E402
import raster_absgrad_ref as R  # noqa: E402
from oracle import raster_oracle as RO  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("shape", R.SCENES, ids=R.SCENE_IDS)
def test_restatement_is_pinned_to_the_oracle(shape):
    """colour, depth and alpha equal RO.render's exactly; the plain sums over pixels equal RO.render_with_grads' px / py gradients
    to 1e-12 of the largest entry (measured: an exact 0 for both)."""
    ref = R.reference(shape)
    sc, aux = ref["sc"], ref["aux"]
    oc, od, oa = ref["oracle"]
    assert torch.equal(ref["color"], oc) and torch.equal(ref["depth"], od) and torch.equal(ref["alpha"], oa)
    *_, grads = RO.render_with_grads(aux["pre"], aux["point_list"], aux["ranges"], sc["bg"], sc["H"], sc["W"], *ref["weights"])
    for c, k in enumerate(("px", "py")):
        err = float((ref["signed_px"][:, c] - grads[k]).abs().max())
        scale = float(grads[k].abs().max())
        print(shape, k, f"max |sum_p dL/de - oracle| = {err:.3e} of {scale:.3e}")
        assert scale > 0 and err <= 1e-12 * scale


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("shape", A.SHAPES, ids=R.SCENE_IDS[:3])
def test_scenes_exercise_the_kernel(shape):
    """>= 2 tile lists longer than 128 entries (more than one staging round; measured 3, 2 and 4 lists, the longest 217, 164 and
    291) and a median abs norm / plain norm of at least 1.5 (measured 4.0, 2.2, 1.9): not a rescaling of the plain statistic."""
    ref = R.reference(shape)
    long_lists = [n for n in ref["lists"] if n > 128]
    an, pn = R.norms(ref)
    touched = pn > 0
    ratio = (an[touched] / pn[touched])
    print(shape, "lists > 128:", len(long_lists), "longest", max(ref["lists"]), "median ratio", float(ratio.median()),
          "share above 2x:", float((ratio > 2).double().mean()))
    assert len(long_lists) >= 2
    assert int(touched.sum()) > shape[0] // 2
    assert float(ratio.median()) >= 1.5
    assert bool((an + 1e-300 >= pn * (1 - 1e-12)).all())            # |sum| <= sum of | |, component-wise hence in norm
    assert float(ref["abs"][~ref["valid"]].abs().max()) == 0.0      # culled Gaussians are in no list
    assert bool((ref["abs"] >= 0).all())
    # without a depth gradient the reference is another one (the depth weights matter)
    nod = R.reference(shape, depth_grad=False)
    assert float((nod["abs"] - ref["abs"]).abs().max()) > 1e-3 * float(ref["abs"].max())


# ---------------------------------------------------------------------------------------------------------------- 3
def test_opaque_scene_exercises_the_early_stop():
    """every opacity 0.99: the pixels saturate and the Gaussians behind get nothing - at most 60 % of the visible ones have a
    non-zero reference value (measured: 308 of 790)"""
    ref = R.reference(R.OPAQUE)
    visible = ref["valid"]
    nz = (ref["abs"].abs().sum(1) > 0) & visible
    print("opaque scene: non-zero", int(nz.sum()), "of", int(visible.sum()), "visible")
    assert int(visible.sum()) > 700
    assert 0 < int(nz.sum()) <= 0.6 * int(visible.sum())


# ---------------------------------------------------------------------------------------------------------------- 4
def test_cancellation():
    """one isotropic Gaussian between four pixels under a constant colour weight: the plain sum cancels, the absolute one does not"""
    ref = R.cancel_reference()
    pre = ref["aux"]["pre"]
    assert abs(float(pre["px"][0]) - 31.5) < 1e-9 and abs(float(pre["py"][0]) - 31.5) < 1e-9
    an, pn = R.norms(ref)
    print("cancellation scene: abs norm", float(an[0]), "plain norm", float(pn[0]))
    assert float(an[0]) > 0
    assert float(pn[0]) <= 1e-9 * float(an[0])


# ---------------------------------------------------------------------------------------------------------------- 5
def declared_symbols():
    text = (ROOT / "include" / "syn3r_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(syn3r_[a-z0-9_]+)\s*\(", text)))


def test_symbols_declared_and_bound():
    from syn3r_amd import _lib
    names = declared_symbols()
    for n in ("syn3r_raster_backward_abs", "syn3r_densification_stats_abs"):
        assert n in names, f"{n} is not declared in include/syn3r_hip.h"
        assert n in _lib.SIGNATURES, f"{n} is not in _lib.SIGNATURES"
    f3d, ab = _lib.SIGNATURES["syn3r_raster_backward_f3d"], _lib.SIGNATURES["syn3r_raster_backward_abs"]
    assert ab[0] is f3d[0] and ab[1] == f3d[1][:-1] + [_lib.c_p, _lib.c_p]        # _f3d's arguments, the buffer, the stream
    st, sa = _lib.SIGNATURES["syn3r_densification_stats"], _lib.SIGNATURES["syn3r_densification_stats_abs"]
    assert len(sa[1]) == len(st[1]) + 2
    # the header's argument lists say the same
    text = (ROOT / "include" / "syn3r_hip.h").read_text()
    decl = re.search(r"int syn3r_raster_backward_abs\((.*?)\);", text, flags=re.S).group(1)
    ref = re.search(r"int syn3r_raster_backward_f3d\((.*?)\);", text, flags=re.S).group(1)
    norm = lambda t: [" ".join(a.split()) for a in t.split(",")]
    assert norm(decl) == norm(ref)[:-1] + ["float* dL_dmeans2D_abs", "void* stream"]
    decl = re.search(r"int syn3r_densification_stats_abs\((.*?)\);", text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in norm(decl)] == ["N", "radii", "viewspace_grad", "abs_grad", "grad_accum", "grad_accum_abs",
                                                               "denom", "max_radii", "stream"]


def test_flags_and_fields():
    from syn3r_amd import launch
    from syn3r_amd.gs import OptimizationParams
    d = OptimizationParams()
    assert d.densify_abs_grad is False and d.densify_abs_grad_threshold == 0.0008
    off = launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x"]))
    assert off.densify_abs_grad is False and off.densify_abs_grad_threshold == 0.0008
    off = launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x", "--densify_abs_grad", "0"]))
    assert off.densify_abs_grad is False
    on = launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x", "--densify_abs_grad", "1"]))
    assert on.densify_abs_grad is True and on.densify_abs_grad_threshold == 0.0008 and on.densify_grad_threshold == d.densify_grad_threshold
    both = launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x", "--densify_abs_grad", "1",
                                                                          "--densify_abs_grad_threshold", "0.002"]))
    assert both.densify_abs_grad is True and both.densify_abs_grad_threshold == 0.002
    thr = launch.apply_trainer_flags(OptimizationParams(), launch.parse(["--scenes", "x", "--densify_abs_grad_threshold", "0.001"]))
    assert thr.densify_abs_grad is False and thr.densify_abs_grad_threshold == 0.001
    for bad in (["--densify_abs_grad", "2"], ["--densify_abs", "1"], ["--densify_abs_grad_thresh", "0.1"]):
        with pytest.raises(SystemExit):
            launch.parse(["--scenes", "x"] + bad)


def test_python_surface_defaults():
    """`abs_grad_out` / `means2D_abs` / `abs_grad` are optional and default to None: the existing calls are untouched"""
    import inspect
    from syn3r_amd import raster
    from syn3r_amd.gs import GaussianModel
    assert inspect.signature(raster.rasterize_backward).parameters["abs_grad_out"].default is None
    assert inspect.signature(raster.GaussianRasterizer.forward).parameters["means2D_abs"].default is None
    assert inspect.signature(GaussianModel.add_densification_stats).parameters["abs_grad"].default is None
    assert list(inspect.signature(raster.rasterize_backward).parameters)[:4] == ["st", "g_color", "g_depth", "g_alpha"]
