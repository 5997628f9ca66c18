"""The LPIPS "fp16x2" precision without a GPU: where the image gradient's error comes from (a float64 emulation with individual
roundings inserted, tests/lpips_split_ref.py), the launcher flag and the constructor's check.

The emulation pins the diagnosis that the mode rests on: the 5-6 % of the fp16 path are NOT the chain of fp16 backward-data
convolutions (whose floor is ~4.4e-4) but the fp16 storage of the FORWARD activations - a post-ReLU map rounded to fp16 perturbs
the next convolution's input by ~3e-4, which flips a few 1e-4 of the ReLU masks per layer, and the gradient of a ReLU network is
discontinuous in exactly those masks.  Stored as fp16 pairs hi + lo the activations are exact to ~2^-22 and the gradient is back
at the floor of its fp16 chain."""
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import lpips_split_ref as R  # noqa: E402

H, W = 64, 96       # float64 autograd through VGG16 takes seconds here


@pytest.fixture(scope="module")
def case():
    torch.manual_seed(0)
    sd = R.seeded_state_dict(R.parameter_shapes(), seed=3)
    a, b = R.images(H, W, H)
    ao = a.double().requires_grad_(True)
    R.LO.lpips(ao, b.double(), sd).backward()
    return sd, a.double(), b.double(), ao.grad.clone()


def _grad(case, **kw):
    sd, a, b, ref = case
    x = a.clone().requires_grad_(True)
    R.emulate(x, b, sd, **kw).backward()
    return R.grad_error(x.grad, ref)


def test_emulation_without_roundings_is_the_oracle(case):
    rel, cos = _grad(case)
    assert rel < 1e-12, rel


def test_fp16_activations_carry_the_gradient_error(case):
    """What the default mode does (fp16 activations, fp16 scaled gradients): 4e-2 .. 8e-2, the 5.4-5.75 % measured on the GPU;
    and the activations alone (gradients exact) give the same figure, the fp16 gradient chain alone 1e-2 of it."""
    rel_both, cos_both = _grad(case, act=R.round_fp16, grad_fp16=True)
    rel_act, _ = _grad(case, act=R.round_fp16, target_act=None)
    rel_grad, cos_grad = _grad(case, grad_fp16=True)
    print(f"fp16 activations + fp16 gradients {rel_both:.3e} (cos {cos_both:.7f}); render branch's activations alone {rel_act:.3e}; "
          f"fp16 gradients alone {rel_grad:.3e} (cos {cos_grad:.9f})")
    assert 4e-2 < rel_both < 8e-2, rel_both
    assert 4e-2 < rel_act < 8e-2, rel_act
    assert rel_grad < 5e-4, rel_grad


def test_split_activations_restore_the_gradient(case):
    """fp16 pairs for the activations of both branches, fp16 scaled gradients (the "fp16x2" mode): below 5e-4."""
    rel, cos = _grad(case, act=R.round_fp16x2, grad_fp16=True)
    rel_exact_grads, _ = _grad(case, act=R.round_fp16x2)
    print(f"fp16x2 activations + fp16 gradients {rel:.3e} (cos {cos:.9f}); gradients exact {rel_exact_grads:.3e}")
    assert rel < 5e-4, rel
    assert rel_exact_grads < rel        # what is left is the fp16 gradient chain, not the activations


def test_launcher_passes_lpips_precision():
    from syn3r_amd import launch
    assert launch.parse(["--scenes", "x"]).lpips_precision == "fp16"
    for v in ("fp16", "fp16x2"):
        a = launch.parse(["--scenes", "x", "--lpips_precision", v])
        assert a.lpips_precision == v
        assert a.ignored_flags == []
    with pytest.raises(SystemExit):
        launch.parse(["--scenes", "x", "--lpips_precision", "fp32"])
    # the tolerated FSGS flags are still tolerated next to it
    b = launch.parse(["--scenes", "x", "--lpips_precision", "fp16x2", "--svd_lpips_weight", "0.5"])
    assert b.lpips_precision == "fp16x2" and b.ignored_flags == ["--svd_lpips_weight", "0.5"]


def test_precision_argument_is_validated():
    from syn3r_amd.gs.lpips import LPIPS
    assert LPIPS().precision == "fp16" and not LPIPS().split
    m = LPIPS(precision="fp16x2")
    assert m.precision == "fp16x2" and m.split and m.parameter_shapes() == LPIPS().parameter_shapes()
    with pytest.raises(ValueError):
        LPIPS(precision="fp32")
    with pytest.raises(ValueError):
        LPIPS(precision="")
