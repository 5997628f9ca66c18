"""Poisoned allocations: what a kernel reads before anything wrote it.

Every wrapper of syn3r_amd allocates outputs and state with `torch.empty*` and scratch through `_lib.workspace()`.  In a short test
process those buffers are fresh and in practice zero; in a long training run the caching allocator and the cached workspaces hand back
stale memory.  `poisoned(monkeypatch, byte)` makes that difference visible: inside the block every new uninitialised tensor (device,
host and pinned host alike) and every cached workspace holds `byte` in every byte, so a result that depends on such a word changes
with the pattern.

    pattern   fp32 / fp16              int32        flags
    0x00      0 / 0 (a fresh process)  0            0
    0xFF      NaN / NaN                -1           255
    0x3C      0.0115 / 1.0586          1010580540   60
(0x3C because fmaxf / fminf and comparisons swallow a NaN; a plausible finite number changes the result instead.)

`run_row` is the table runner of tests/test_uninit_gpu.py; it lives here so that tests/test_poison_cpu.py can show, without a GPU,
that it reports a leaky op.  A helper module, not a conftest: nothing here changes how the suite is collected or run.
"""
from __future__ import annotations

import contextlib
from typing import Callable, NamedTuple, Optional, Sequence

import torch

PATTERNS = (0x00, 0xFF, 0x3C)

_PATCHED = ("empty", "empty_like", "empty_strided")


def fill_bytes(t: torch.Tensor, byte: int, _empty=torch.empty) -> torch.Tensor:
    """Set every byte of `t`'s storage to `byte` (any dtype, any rank, 0-dim included); returns `t`."""
    if not isinstance(t, torch.Tensor) or t.device.type == "meta" or t.is_sparse:
        return t
    st = t.untyped_storage()
    if st.nbytes() == 0:
        return t
    raw = _empty(0, dtype=torch.uint8, device=t.device).set_(st)
    raw.fill_(int(byte))
    return t


@contextlib.contextmanager
def poisoned(monkeypatch, byte: int):
    """While active: `torch.empty`, `torch.empty_like`, `torch.empty_strided` and `Tensor.new_empty` return tensors whose every byte
    is `byte`, and the buffers already in `syn3r_amd._lib._ws_cache` were filled with it on entry.  Restored on exit, also after an
    exception (pytest's `monkeypatch.context()` undoes the patches of the block alone)."""
    if not 0 <= int(byte) <= 255:
        raise ValueError("poison pattern must be one byte")
    from syn3r_amd import _lib
    orig_empty = torch.empty

    def wrap(fn):
        def poisoned_alloc(*args, **kwargs):
            return fill_bytes(fn(*args, **kwargs), byte, orig_empty)
        poisoned_alloc.__name__ = getattr(fn, "__name__", "empty")
        poisoned_alloc.__wrapped__ = fn
        return poisoned_alloc

    for buf in list(_lib._ws_cache.values()):
        fill_bytes(buf, byte, orig_empty)
    with monkeypatch.context() as m:
        for name in _PATCHED:
            m.setattr(torch, name, wrap(getattr(torch, name)))
        m.setattr(torch.Tensor, "new_empty", wrap(torch.Tensor.new_empty))
        yield


class Row(NamedTuple):
    """One op of the sweep.  `run(dev)` goes through the public Python surface and returns a tuple of output tensors; `check(outs)`
    is the op's reference check, at the tolerances of its own test module (it raises AssertionError); `repeatable`: the op's outputs
    are bit-identical from run to run (no float atomics), so they are compared bit for bit across the patterns; `finite_ref`
    (optional): per output a bool tensor, or None for 'everywhere', saying where the reference is finite."""
    name: str
    run: Callable
    repeatable: bool
    check: Optional[Callable] = None
    finite_ref: Optional[Callable] = None


def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous()
    if t.numel() == 0:
        return torch.zeros(0, dtype=torch.uint8)
    return t.reshape(-1).view(torch.uint8).cpu()


def run_row(row: Row, monkeypatch, dev, patterns: Sequence[int] = PATTERNS) -> dict:
    """Run `row` once under each pattern, each in a fresh `poisoned` block.  Asserts that every output is finite where the reference
    is, that the row's reference check passes under every pattern and, for repeatable rows, that all outputs are bit-identical across
    the patterns.  Returns {pattern: outputs}."""
    results = {}
    for byte in patterns:
        with poisoned(monkeypatch, byte):
            outs = tuple(row.run(dev))
            if dev is not None and getattr(dev, "type", "cpu") == "cuda":
                torch.cuda.synchronize(dev)
            results[byte] = outs
            where = row.finite_ref(outs) if row.finite_ref is not None else (None,) * len(outs)
            for k, (o, w) in enumerate(zip(outs, where)):
                if isinstance(o, torch.Tensor) and o.is_floating_point():
                    ok = torch.isfinite(o)
                    if w is not None:
                        ok = ok | ~w.to(o.device)
                    assert bool(ok.all()), f"{row.name}: output {k} is not finite under pattern 0x{byte:02X} ({int((~ok).sum())} entries)"
            if row.check is not None:            # (inside the block: a check may run the op again, e.g. an existing test function)
                try:
                    row.check(outs)
                except AssertionError as e:
                    raise AssertionError(f"{row.name}: reference check failed under pattern 0x{byte:02X}: {e}") from e
    if row.repeatable:
        base = results[patterns[0]]
        for byte in patterns[1:]:
            assert len(results[byte]) == len(base), f"{row.name}: output count differs under pattern 0x{byte:02X}"
            for k, (a, b) in enumerate(zip(base, results[byte])):
                if not isinstance(a, torch.Tensor):
                    assert a == b, f"{row.name}: output {k} differs between patterns 0x{patterns[0]:02X} and 0x{byte:02X}"
                    continue
                assert a.shape == b.shape and a.dtype == b.dtype, f"{row.name}: output {k} changes shape or type with the pattern"
                ba, bb = _bits(a), _bits(b)
                same = torch.equal(ba, bb)
                assert same, (f"{row.name}: output {k} differs between patterns 0x{patterns[0]:02X} and 0x{byte:02X} "
                              f"({int((ba != bb).sum())} of {ba.numel()} bytes): it depends on memory nobody wrote")
    return results
