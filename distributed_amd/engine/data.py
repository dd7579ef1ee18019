"""Device-resident input pipeline.

The whole training set lives in device memory (MNIST: 60000x784 fp32 = 188 MB of
288 GB HBM), a per-epoch permutation is generated from a seed shared by all ranks,
and each rank reads its rows of global batch ``s`` as
``perm[s*global_batch + rank*per_replica : ... + per_replica]`` — deterministic,
disjoint per-rank sharding of every global batch (the reference lets tf.distribute
auto-shard, README.md:127-132; progbar counts global samples, README.md:413).
"""
from __future__ import annotations

import numpy as np
import torch


_BASE_SEED = 0x5EED


def as_u8_over_255(x: np.ndarray):
    """uint8 array k if every element of ``x`` is exactly float32(k/255) (e.g. MNIST's
    ``x / 255.0``), else None.  The fused kernels then stage k/255.f, which is bitwise
    float32(k/255.0), from 4x fewer bytes."""
    if not np.issubdtype(x.dtype, np.floating):
        return None
    k = np.rint(x * 255.0)
    if k.min() < 0 or k.max() > 255:
        return None
    ku8 = k.astype(np.uint8)
    if not np.array_equal((ku8 / 255.0).astype(np.float32), x.astype(np.float32)):
        return None
    return ku8


class DataFeed:
    def __init__(self, x, y, device: torch.device, flatten: bool = False, allow_u8: bool = False, w=None):
        self._key = (id(x), id(y), len(x))  # what a later bind compares its arrays with (built_from)
        x = np.asarray(x)
        y = np.asarray(y)
        if len(x) != len(y):
            raise ValueError(f"x has {len(x)} rows but y has {len(y)}")
        self.n = int(len(x))
        # per-sample loss weights (keras/utils.py resolve_sample_weights): fp32 [n] on the
        # device in dataset order, indexed like x and y; the host copy tells whether a later
        # bind brings the same weights
        self.w, self.w_host = None, None
        if w is not None:
            self.w_host = np.array(w, dtype=np.float32).reshape(-1)
            if self.w_host.shape[0] != self.n:
                raise ValueError(f"x has {self.n} rows but there are {self.w_host.shape[0]} sample weights")
            self.w = torch.from_numpy(self.w_host).to(device)
        u8 = as_u8_over_255(x) if allow_u8 else None
        self.x_u8 = u8 is not None
        xt = torch.from_numpy(np.ascontiguousarray(u8 if self.x_u8 else x, dtype=np.uint8 if self.x_u8 else np.float32))
        if flatten:
            xt = xt.reshape(self.n, -1)
        self.x = xt.to(device)
        if y.ndim > 1 and y.shape[-1] > 1:  # one-hot / dense targets
            self.y = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(device)
        else:  # class ids
            self.y = torch.from_numpy(np.ascontiguousarray(y.reshape(self.n), dtype=np.int64)).to(device).to(
                torch.int32)
        self.perm = torch.arange(self.n, dtype=torch.int32, device=device)
        self.device = device

    def built_from(self, x, y, w=None) -> bool:
        """This feed was built from these very arrays (by identity and length; a native
        engine passes ``x`` after its ``np.asarray``) and the same weights (by value)."""
        return self._key == (id(x), id(y), len(x)) and self.same_weights(w)

    def alloc_epoch(self) -> None:
        """x, y (and the weights) in epoch order, for the engines that read batches at a device
        cursor.  Once per feed: captured graphs and the fused trainer hold the addresses."""
        self.x_ep = torch.empty_like(self.x)
        self.y_ep = torch.empty_like(self.y)
        self.w_ep = torch.empty_like(self.w) if self.w is not None else None

    def fill_epoch(self) -> None:
        """Materialise the order of the last ``set_epoch`` once (one gather per epoch instead
        of an index indirection on every step's critical path)."""
        perm = self.perm.long()
        torch.index_select(self.x, 0, perm, out=self.x_ep)
        torch.index_select(self.y, 0, perm, out=self.y_ep)
        if self.w_ep is not None:
            torch.index_select(self.w, 0, perm, out=self.w_ep)

    def same_weights(self, w) -> bool:
        """``w`` (None or an array) is what this feed was built with."""
        if w is None or self.w_host is None:
            return w is None and self.w_host is None
        w = np.asarray(w, dtype=np.float32).reshape(-1)
        return w.shape == self.w_host.shape and bool(np.array_equal(w, self.w_host))

    def set_epoch(self, epoch: int, shuffle: bool = True, seed: int = None) -> None:
        if not shuffle:
            p = torch.arange(self.n, dtype=torch.int32)
        else:
            g = torch.Generator()
            g.manual_seed(int(seed if seed is not None else _BASE_SEED) * 7919 + int(epoch))
            p = torch.randperm(self.n, generator=g).to(torch.int32)
        self.perm.copy_(p.to(self.device))

    def batch_indices(self, step: int, global_batch: int, row0: int, per_replica: int) -> torch.Tensor:
        lo = step * global_batch + row0
        hi = min(lo + per_replica, self.n)
        lo = min(lo, self.n)
        return self.perm[lo:hi].long()
