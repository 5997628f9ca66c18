"""The trainer's host code launches what it launched before it was split into modules: per step route and option set, the kernels
of three `train_step` calls and their counts equal the table recorded on the parent commit (tests/data/trainer_launches.json,
written by tests/trainer_launches.py there; the recording is never taken from the tree under test)."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import trainer_launches as TL  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table():
    return TL.expected()


def test_the_table_covers_every_configuration(table):
    """All eight configurations are in the table, and the six without density control survive whole (nothing left out)"""
    assert sorted(table["launches"]) == sorted(TL.key(*c) for c in TL.CONFIGS)
    assert all(k.endswith("/density") for k in table["left_out"]), table["left_out"]
    for k, row in table["launches"].items():
        assert row.get("k_adam_multi") == TL.STEPS and row.get("k_render") == TL.STEPS and row.get("k_render_bwd") == TL.STEPS, k


@pytest.mark.parametrize("route,name", TL.CONFIGS, ids=[TL.key(*c) for c in TL.CONFIGS])
def test_same_launches_as_the_parent(route, name, gpu, table):
    k = TL.key(route, name)
    left_out = set(table["left_out"].get(k, ()))
    got = {kernel: calls for kernel, calls in TL.launches(gpu, route, name).items() if kernel not in left_out}
    assert got == table["launches"][k]
