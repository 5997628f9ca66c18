"""`FusedAdam`: torch.optim.Adam's update with one launch per eight parameter tensors (`syn3r_adam_step_multi[_rows]`,
csrc/train.hip)."""
from __future__ import annotations

from typing import Iterable, List, NamedTuple

import torch

from ... import _lib as L


class _AdamItem(NamedTuple):
    """One tensor of a `FusedAdam.step` launch table; `row_len` 0: a plain tensor (`lr_tail`, `head_len` unused)."""
    param: torch.Tensor
    grad: torch.Tensor
    state: dict
    lr: float
    eps: float
    lr_tail: float
    row_len: int
    head_len: int


class FusedAdam:
    """`torch.optim.Adam(param_groups, eps=...)` (no weight decay / amsgrad) with one kernel per parameter tensor.
    Keeps torch's `param_groups` / `state` layout so checkpoints and lr schedules written for the torch optimiser
    keep working.
    A group may carry `lr_tail`, `row_len` and `head_len`: its tensors are rows of `row_len` floats whose first `head_len` take
    `lr` and the rest `lr_tail` (`syn3r_adam_step_multi_rows`: the published 3DGS f_dc / f_rest groups as ONE [N, M, 3] tensor
    with row_len = 3 M, head_len = 3).  `row_len` 0 or absent: a plain group."""

    def __init__(self, param_groups: Iterable[dict], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        self.param_groups: List[dict] = []
        for g in param_groups:
            g = dict(g)
            g["params"] = list(g["params"])
            g.setdefault("lr", lr)
            g.setdefault("betas", betas)
            g.setdefault("eps", eps)
            self.param_groups.append(g)
        self.state: dict = {}

    def zero_grad(self, set_to_none: bool = True):
        for g in self.param_groups:
            for p in g["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    @torch.no_grad()
    def step(self):
        """One update of every parameter that has a gradient: ONE launch per (beta1, beta2) and up to 8 tensors
        (`syn3r_adam_step_multi`; the trainer's five / six groups share their betas), element for element `torch.optim.Adam`.
        A chunk with a tensor of a row-split group goes through `syn3r_adam_step_multi_rows` (the plain tensors ride along with
        row_len = 0); a chunk without one takes `syn3r_adam_step_multi` as before."""
        import ctypes as C
        lib = L.load()
        batches: dict = {}
        for g in self.param_groups:
            b1, b2 = g["betas"]
            row_len = int(g.get("row_len") or 0)
            lr_tail, head_len = (float(g["lr_tail"]), int(g["head_len"])) if row_len else (0.0, 0)
            for p in g["params"]:
                if p.grad is None:
                    continue
                L.require_gpu(p)
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError("FusedAdam: parameters must be contiguous float32")
                st = self.state.get(p)
                if st is None:
                    st = self.state[p] = {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
                st["step"] += 1
                grad = p.grad.contiguous()
                batches.setdefault((float(b1), float(b2), p.device), []).append(
                    _AdamItem(p, grad, st, float(g["lr"]), float(g["eps"]), lr_tail, row_len, head_len))
        for (b1, b2, dev), items in batches.items():
            for k0 in range(0, len(items), 8):
                chunk = items[k0:k0 + 8]
                n = len(chunk)
                ptrs = lambda sel: (C.c_void_p * n)(*[sel(it).data_ptr() for it in chunk])
                arr = lambda ctype, sel: (ctype * n)(*[sel(it) for it in chunk])
                tables = (n, ptrs(lambda it: it.param), ptrs(lambda it: it.grad), ptrs(lambda it: it.state["exp_avg"]),
                          ptrs(lambda it: it.state["exp_avg_sq"]), arr(C.c_longlong, lambda it: it.param.numel()),
                          arr(C.c_float, lambda it: it.lr))
                tail = (b1, b2, arr(C.c_float, lambda it: it.eps), arr(C.c_int, lambda it: int(it.state["step"])), L.stream_ptr(dev))
                if any(it.row_len for it in chunk):
                    rc = lib.syn3r_adam_step_multi_rows(*tables, arr(C.c_float, lambda it: it.lr_tail), arr(C.c_int, lambda it: it.row_len),
                                                        arr(C.c_int, lambda it: it.head_len), *tail)
                    L.check(rc, "adam_step_multi_rows")
                else:
                    rc = lib.syn3r_adam_step_multi(*tables, *tail)
                    L.check(rc, "adam_step_multi")
