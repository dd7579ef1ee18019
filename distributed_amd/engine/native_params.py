"""The flat parameter layout of the native engines: every variable a plan reads, back to back
in one fp32 master buffer with a bf16 shadow (and, for training, the gradient buffer and the
optimizer slots in the same layout)."""
from __future__ import annotations

import numpy as np
import torch

from ..ops import hip as H
from .native_plan import _pad8, reg_rows


class FlatParams:
    """``variables`` laid out flat: fp32 masters ``P`` and their bf16 shadow ``Pb``.  Every
    variable starts on an 8-element boundary: 16-byte aligned bf16 / 32-byte aligned fp32
    views for the kernels' vector accesses.  ``train``: also the gradient buffer ``G`` (+ the
    8-word metric tail) and a flat ``S[name]`` per named optimizer slot, and the variables
    are rebound to their views of ``P``; otherwise ``P`` is a copy the owner refreshes."""

    def __init__(self, variables, device, train: bool = False, slots=()):
        self.vars = variables
        self.sizes = [int(np.prod(v.shape)) for v in variables]
        self.offsets, off = [], 0
        for sz in self.sizes:
            self.offsets.append(off)
            off = _pad8(off + sz)
        self.n = n = off
        self.P = torch.zeros(n, dtype=torch.float32, device=device)
        self.Pb = torch.zeros(n, dtype=torch.bfloat16, device=device)
        self.G = torch.zeros(n + 8, dtype=torch.float32, device=device) if train else None  # + metric tail
        self.S = {nm: torch.zeros(n, dtype=torch.float32, device=device) for nm in slots if nm}
        self.views, self.bviews, self.gviews = {}, {}, {}
        for v, sz, off in zip(variables, self.sizes, self.offsets):
            self.views[id(v)] = self.P[off:off + sz].view(v.shape)
            self.bviews[id(v)] = self.Pb[off:off + sz].view(v.shape)
            if train:
                v._rebind(self.P[off:off + sz].view(v.shape))
                self.gviews[id(v)] = self.G[off:off + sz].view(v.shape)
        # weight regularizers: the segment table of opt_step / reg_penalty, built once (None:
        # no regularizer -- nothing is launched for them and opt_step runs without the table)
        self.reg_rows = reg_rows(variables, self.offsets)
        self.reg_tab = H.reg_table(self.reg_rows, device) if self.reg_rows else None
        self.reg_scratch = H.reg_scratch(n, device) if self.reg_rows else None

    def view(self, var):
        """The fp32 master view of ``var`` (None for None: an absent bias / gamma / beta)."""
        return self.views[id(var)] if var is not None else None

    def bview(self, var):
        return self.bviews[id(var)] if var is not None else None

    def gview(self, var):
        return self.gviews[id(var)] if var is not None else None
