"""Generic engine: any Keras model, per-layer ops, autograd backward, flat-bucket DP.

Per step (per replica): gather the local rows of the global batch from the
device-resident feed, forward, per-sample loss, ``sum / global_batch`` so that a SUM
all-reduce gives the global-mean gradient, write all gradients into ONE
flat fp32 buffer whose tail carries [loss_sum, count, metric sums...] (SURVEY.md D6:
one collective per step for grads + metrics), all-reduce it, apply the optimizer on the
flat master buffer, and accumulate the metric tail on device (no host sync per step).
"""
from __future__ import annotations

import numpy as np
import torch

from ..keras import backend as K
from ..keras.layers import augment_seeds
from .base import Engine
from .data import DataFeed


class GenericEngine(Engine):
    name = "generic"

    def __init__(self, model, strategy, per_replica_batch, global_batch):
        super().__init__(model, strategy, per_replica_batch, global_batch)
        self.vars = model.trainable_weights
        self.sizes = [int(np.prod(v.shape)) for v in self.vars]
        self.n = int(sum(self.sizes))
        dev = self.device
        self.P = torch.zeros(self.n, dtype=torch.float32, device=dev)
        off = 0
        self.leaves = []
        for v, sz in zip(self.vars, self.sizes):
            view = self.P[off:off + sz].view(v.shape)
            with torch.no_grad():
                view.copy_(v.value.detach().to(dev, torch.float32))
            leaf = torch.empty(0, device=dev)
            leaf.data = view
            leaf.requires_grad_(True)
            v._t = leaf
            self.leaves.append(leaf)
            off += sz
        self.loss = model.loss
        self.metric_objs = model.compiled_metrics
        self.ntail = 2 + len(self.metric_objs)
        self.G = torch.zeros(self.n + self.ntail, dtype=torch.float32, device=dev)
        self.acc = torch.zeros(self.ntail, dtype=torch.float64, device=dev)
        model.optimizer.ensure_slots(self.n, dev)
        opt = model.optimizer
        if opt._iter_source is not None:
            # a native engine counted the iterations on its device: apply_flat counts on the
            # host, and a learning-rate schedule (or Adam's t) continues from that count
            opt._iterations = int(opt.iterations)
            opt._iter_source = None
        # mirrored variables: replicas start from worker 0's values
        if self.world > 1:
            comm = strategy.communicator
            comm.broadcast_(self.P, 0)
            for w in model.non_trainable_weights:
                comm.broadcast_(w.value.data if w.value.requires_grad else w.value, 0)
        self.feed = None
        self.step_in_epoch = 0
        self._plan_buckets()
        self._plan_regularizers()
        # gradient clipping (keras/optimizers.py): read once, when the engine is built
        self.clip_mode, self.clip_c = model.optimizer.clipping()
        self.aug_seeds = augment_seeds(model)  # RandomFlip / RandomCrop: effective seeds, fixed per model

    def _plan_regularizers(self):
        """Weight penalties (keras/regularizers.py).  L1L2 on a trainable variable: a row
        (offset, size, l1, l2) of ``reg_table`` over the flat buffer, closed form
        (ops/reference.py reg_grad / reg_penalty).  Any other callable: evaluated and
        differentiated with torch.  A frozen layer's regularizer adds to the loss only."""
        from ..keras import regularizers as _regs

        idx = {id(v): i for i, v in enumerate(self.vars)}
        self.reg_table, self.reg_other, self.reg_frozen = [], [], []
        for v, r in self.model._regularized():
            i, co = idx.get(id(v)), _regs.coefficients(r)
            if i is None:
                self.reg_frozen.append((v, r))
            elif co is not None:
                self.reg_table.append((self.offs[i], self.sizes[i], co[0], co[1]))
            else:
                self.reg_other.append((i, r))
        self.regularized = bool(self.reg_table or self.reg_other or self.reg_frozen)

    @torch.no_grad()
    def _reg_penalty(self):
        """R at the current weights (fp32 scalar on the device)."""
        from ..ops import reference

        r = reference.reg_penalty(self.P, self.reg_table)
        for i, f in self.reg_other:
            r = r + f(self.leaves[i].detach()).float()
        for v, f in self.reg_frozen:
            r = r + f(v.value.detach()).float().to(r.device)
        return r

    def _add_reg_grad(self, g):
        """g (the all-reduced flat gradient) += dR/dw: once per step, whatever the world size."""
        from ..ops import reference

        with torch.no_grad():
            if self.reg_table:
                g += reference.reg_grad(self.P, self.reg_table)
        for i, f in self.reg_other:
            (d,) = torch.autograd.grad(f(self.leaves[i]), self.leaves[i], allow_unused=True)
            if d is not None:
                with torch.no_grad():
                    g[self.offs[i]:self.offs[i] + self.sizes[i]] += d.reshape(-1)

    def _plan_buckets(self):
        """Gradient buckets (SURVEY.md §3.3 / N3'): contiguous ranges of G filled from the
        last layer backwards, the metric tail in the first one.  During backward each
        parameter's gradient is copied into G by a hook; when a bucket is complete its
        all-reduce starts asynchronously while autograd computes the earlier layers."""
        from ..utils import env

        self.bucketed = self.world > 1 and env.get_float("DAMD_BUCKET_MB", 8.0) > 0
        self.allreduce_kind = ("none" if self.world == 1 else
                               f"{self.strategy.communicator.name}{'-bucketed' if self.bucketed else ''}")
        limit = max(1, int(env.get_float("DAMD_BUCKET_MB", 8.0) * 2**20 / 4))
        offs, off = [], 0
        for sz in self.sizes:
            offs.append(off)
            off += sz
        self.offs = offs
        buckets, cur, n = [], [], 0
        for i in reversed(range(len(self.sizes))):
            cur.append(i)
            n += self.sizes[i]
            if n >= limit:
                buckets.append(cur)
                cur, n = [], 0
        if cur:
            buckets.append(cur)
        self.buckets = []
        for bi, idxs in enumerate(buckets):
            lo = min(offs[i] for i in idxs)
            hi = self.n + self.ntail if bi == 0 else max(offs[i] + self.sizes[i] for i in idxs)
            self.buckets.append((lo, hi, set(idxs)))
        self.bucket_of = {i: b for b, (_, _, idxs) in enumerate(self.buckets) for i in idxs}

    def bind(self, x, y, w=None):
        if self.feed is None or not self.feed.built_from(x, y, w):
            self.feed = DataFeed(x, y, self.device, w=w)
        return self.feed

    def start_epoch(self, epoch, shuffle):
        self.feed.set_epoch(epoch, shuffle, self.shuffle_seed)
        self.step_in_epoch = 0
        self.acc.zero_()

    def _tick(self, name):
        ph = getattr(self, "_phases", None)
        if ph is None:
            return
        import time

        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        t = time.perf_counter()
        ph[name] = ph.get(name, 0.0) + (t - self._t_last) * 1e3
        self._t_last = t

    def phase_times(self, n_steps: int) -> dict:
        """Host-timed phases (device synchronised at each point): forward + loss, backward
        (bucketed all-reduces already launched inside it), the wait for the all-reduce,
        optimizer."""
        import time

        self.sync()
        self._phases = {}
        try:
            for _ in range(n_steps):
                left = self.feed.n // max(self.global_batch, 1) - self.step_in_epoch
                if left <= 0:
                    self.start_epoch(0, False)
                self._t_last = time.perf_counter()
                self._one_step()
            out = {k: v / max(n_steps, 1) for k, v in self._phases.items()}
        finally:
            self._phases = None
        out["step"] = sum(out.values())
        out["allreduce_kind"] = self.allreduce_kind
        return out

    def _one_step(self):
        feed, model = self.feed, self.model
        s = self.step_in_epoch
        idx = feed.batch_indices(s, self.global_batch, self.rank * self.per_replica, self.per_replica)
        gstart = s * self.global_batch
        gcount = max(0, min(self.global_batch, feed.n - gstart))
        G = self.G
        G.zero_()
        works = None
        if idx.numel() > 0 and gcount > 0:
            xb, yb = feed.x[idx], feed.y[idx]
            # input augmentation draws from (seed, t, global batch slot): what the native
            # engines read from Ctrl::cur3 and Ctrl::row0 + r (keras/backend.py AugmentContext)
            row0 = self.rank * self.per_replica
            with K.AugmentContext(int(model.optimizer.iterations) + 1, np.arange(row0, row0 + idx.numel()),
                                  self.aug_seeds):
                out = model(xb, training=True)
            ls = self.loss.per_sample(yb, out)
            if feed.w is not None:
                # sample / class weights: sum w_i l_i over the rows that exist; the count and
                # the metrics stay unweighted (Keras SUM_OVER_BATCH_SIZE)
                ls = ls * feed.w[idx]
            loss = ls.sum() * (1.0 / gcount)
            self._tick("forward")
            with torch.no_grad():
                G[self.n] = ls.detach().sum()
                if self.regularized:  # the SUM all-reduce then yields R * (global rows)
                    G[self.n] += self._reg_penalty() * float(idx.numel())
                G[self.n + 1] = float(idx.numel())
                for i, m in enumerate(self.metric_objs):
                    G[self.n + 2 + i] = m.per_sample(yb, out.detach()).sum()
            if self.bucketed:
                works = self._backward_bucketed(loss)
            else:
                grads = torch.autograd.grad(loss, self.leaves, allow_unused=True)
                for g, sz, off in zip(grads, self.sizes, self.offs):
                    if g is not None:
                        G[off:off + sz].copy_(g.reshape(-1))
        elif self.bucketed:
            # a replica with no rows (short last batch) still issues the same bucket
            # sequence as the others: one all-reduce per bucket, in bucket order
            comm = self.strategy.communicator
            works = [comm.allreduce_async(G[lo:hi], "sum") for (lo, hi, _) in self.buckets]
        self._tick("backward")
        if works is not None:
            for w in works:
                w.wait()
        elif self.world > 1:
            self.strategy.communicator.allreduce_(G, "sum")
        self._tick("allreduce")
        if self.regularized:
            self._add_reg_grad(G[: self.n])
        if self.clip_mode is not None:
            # Keras clipping of what the update rule consumes: after the exchange, with dR/dw
            from ..ops import reference

            reference.clip_grad(G[: self.n], list(zip(self.offs, self.sizes)), self.clip_mode, self.clip_c)
        self.model.optimizer.apply_flat(self.P, G[: self.n])
        self.acc += G[self.n:].double()
        self.step_in_epoch += 1
        self._tick("optimizer")

    def _backward_bucketed(self, loss):
        comm, G = self.strategy.communicator, self.G
        left = [set(idxs) for (_, _, idxs) in self.buckets]
        works = [None] * len(self.buckets)

        def launch(b):
            lo, hi, _ = self.buckets[b]
            works[b] = comm.allreduce_async(G[lo:hi], "sum")

        nxt = [0]

        def launch_ready():
            # buckets start strictly in index order (a complete bucket waits for the
            # earlier ones), so every rank issues the identical collective sequence even
            # if autograd finishes parameters in a different order
            while nxt[0] < len(self.buckets) and not left[nxt[0]]:
                launch(nxt[0])
                nxt[0] += 1

        def make_hook(i):
            def hook(g):
                off, sz = self.offs[i], self.sizes[i]
                with torch.no_grad():
                    G[off:off + sz].copy_(g.reshape(-1))
                left[self.bucket_of[i]].discard(i)
                launch_ready()
                return g
            return hook

        handles = [leaf.register_hook(make_hook(i)) for i, leaf in enumerate(self.leaves)]
        try:
            torch.autograd.backward(loss, inputs=self.leaves)
        finally:
            for h in handles:
                h.remove()
        for b in range(nxt[0], len(self.buckets)):  # parameters that received no gradient
            launch(b)
        for leaf in self.leaves:
            leaf.grad = None
        return works

    def run(self, n_steps):
        for _ in range(n_steps):
            self._one_step()

    def metrics(self):
        a = self.acc.cpu().tolist()
        cnt = a[1] if a[1] else 1.0
        out = {"loss": a[0] / cnt}
        for i, m in enumerate(self.metric_objs):
            out[m.name] = a[2 + i] / cnt
        out["_count"] = a[1]
        return out

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
