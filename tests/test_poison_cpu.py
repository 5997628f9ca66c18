"""tests/poison.py on the CPU: the bytes of fresh tensors under each pattern, restoration, and that the table runner of
tests/test_uninit_gpu.py reports an op that returns memory nobody wrote."""
import numpy as np
import pytest
import torch

from poison import PATTERNS, Row, fill_bytes, poisoned, run_row

DTYPES = [torch.float32, torch.float16, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool]


def raw_bytes(t):
    return np.frombuffer(bytes(t.untyped_storage().tolist()), dtype=np.uint8) if t.untyped_storage().nbytes() else np.zeros(0, np.uint8)


@pytest.mark.parametrize("byte", PATTERNS)
def test_fresh_tensors_hold_the_pattern(byte, monkeypatch):
    like = torch.zeros(3, 5)
    with poisoned(monkeypatch, byte):
        for dt in DTYPES:
            made = [torch.empty(7, 3, dtype=dt), torch.empty((), dtype=dt), torch.empty(0, dtype=dt),
                    torch.empty_like(like, dtype=dt), torch.empty_strided((4, 3), (1, 4), dtype=dt),
                    like.new_empty((2, 9), dtype=dt), like.new_empty((), dtype=dt)]
            for t in made:
                b = raw_bytes(t)
                assert b.size == t.untyped_storage().nbytes() and (b == byte).all(), (dt, tuple(t.shape), byte)
            assert made[1].dim() == 0 and made[4].stride() == (1, 4) and made[3].shape == like.shape
        # the values of the issue's table
        f32, f16, i32, flag = (torch.empty(4, dtype=d) for d in (torch.float32, torch.float16, torch.int32, torch.uint8))
    if byte == 0x00:
        assert (f32 == 0).all() and (f16 == 0).all() and (i32 == 0).all() and (flag == 0).all()
    elif byte == 0xFF:
        assert torch.isnan(f32).all() and torch.isnan(f16).all() and (i32 == -1).all() and (flag == 255).all()
    else:
        assert abs(float(f32[0]) - 0.0115) < 1e-4 and abs(float(f16[0]) - 1.0586) < 1e-3
        assert (i32 == 1010580540).all() and (flag == 0x3C).all()


def test_cached_workspaces_are_filled_on_entry(monkeypatch):
    from syn3r_amd import _lib
    key = ("cpu-selftest", 0, "poison")
    buf = torch.zeros(300, dtype=torch.uint8)
    monkeypatch.setitem(_lib._ws_cache, key, buf)
    with poisoned(monkeypatch, 0x3C):
        assert _lib._ws_cache[key] is buf and (buf == 0x3C).all()
    with poisoned(monkeypatch, 0xFF):
        assert (buf == 0xFF).all()


def test_restored_after_the_block_and_after_an_exception(monkeypatch):
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    now = lambda: (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with poisoned(monkeypatch, 0xFF):
        assert all(a is not b for a, b in zip(now(), before))
    assert all(a is b for a, b in zip(now(), before))
    with pytest.raises(RuntimeError, match="inside"):
        with poisoned(monkeypatch, 0x3C):
            assert torch.empty is not before[0]
            raise RuntimeError("inside")
    assert all(a is b for a, b in zip(now(), before))
    # nested blocks unwind one at a time
    with poisoned(monkeypatch, 0x3C):
        with poisoned(monkeypatch, 0xFF):
            assert torch.isnan(torch.empty(2)).all()
        assert abs(float(torch.empty(2)[0]) - 0.0115) < 1e-4
    assert all(a is b for a, b in zip(now(), before))
    with pytest.raises(ValueError):
        with poisoned(monkeypatch, 256):
            pass
    assert fill_bytes(torch.zeros(()), 0xFF).isnan()


# The "op": the running sum of 14 numbers in a buffer of 16 whose two padding words are specified to be zero (as the gradient rows of
# culled Gaussians are).  The leaky form never writes the last `skip_last` of them: right in a fresh process, wrong on stale memory.
_EXPECT = np.concatenate([np.cumsum(np.arange(14, dtype=np.float32)), np.zeros(2, np.float32)])


def _cumsum_ref(outs):
    np.testing.assert_allclose(outs[0].numpy(), _EXPECT, rtol=0, atol=0)


def _clean_op(dev):
    out = torch.empty(16)
    out.copy_(torch.from_numpy(_EXPECT))
    return (out,)


def _leaky_op(skip_last):
    def op(dev):
        out = torch.empty(16)
        n = 16 - skip_last
        out[:n] = torch.from_numpy(_EXPECT)[:n]
        return (out,)
    return op


def test_runner_passes_a_clean_op_and_reports_a_leaky_one(monkeypatch):
    res = run_row(Row("clean", _clean_op, True, _cumsum_ref), monkeypatch, None)
    assert sorted(res) == sorted(PATTERNS)
    # the unwritten word is NaN under 0xFF: the finite check names the row and the pattern
    with pytest.raises(AssertionError, match=r"leaky: output 0 is not finite under pattern 0xFF"):
        run_row(Row("leaky", _leaky_op(1), True, None), monkeypatch, None)
    # with a reference check, already the finite pattern that is not zero fails it ...
    with pytest.raises(AssertionError, match=r"leaky: reference check failed under pattern 0x3C"):
        run_row(Row("leaky", _leaky_op(1), True, _cumsum_ref), monkeypatch, None, patterns=(0x00, 0x3C))
    # ... and without one the bit comparison across the patterns does
    with pytest.raises(AssertionError, match=r"leaky: output 0 differs between patterns 0x00 and 0x3C \(4 of 64 bytes\)"):
        run_row(Row("leaky", _leaky_op(1), True, None), monkeypatch, None, patterns=(0x00, 0x3C))
    # an op that is not bit-compared still has to pass its reference check
    with pytest.raises(AssertionError, match="reference check failed"):
        run_row(Row("leaky", _leaky_op(2), False, _cumsum_ref), monkeypatch, None, patterns=(0x00, 0x3C))
    # the zero pattern alone is what the suite saw so far: the leak passes, reference check and all
    run_row(Row("leaky", _leaky_op(2), True, _cumsum_ref), monkeypatch, None, patterns=(0x00,))
    assert torch.empty is run_row.__globals__["torch"].empty
