"""Native inference: ``predict`` / ``evaluate`` through the native forward plan.

The reference scores its trained model on a held-out split (README.md:286-290, 369-373:
``model.evaluate`` / ``predict`` after ``fit``; ``fit(validation_split=...)`` evaluates
every epoch).  Here that runs on the same lowered plan as training
(:class:`~distributed_amd.engine.native_graph.NativeGraphEngine`), forward only:

* the inputs of the whole call are uploaded once (uint8 or fp32 rows; 288 GB of HBM holds
  any evaluation split whole) and ``gather_batch`` cuts batch ``cursor`` on the device;
* BatchNorm runs with the MOVING statistics: ``bn_infer_st`` turns them into the same
  (mean, invstd, scale, shift) rows the training plan derives from batch statistics, so
  the fused BN / residual / stem-pool kernels are reused unchanged; Dropout is identity; an
  input prefix (ZeroPadding2D / RandomCrop / RandomFlip) runs its ``augment`` launch in
  inference mode: pads as in training, crops centred, no flips;
* one step = gather -> forward -> (``logits_store`` or, for a softmax output,
  ``softmax_store`` | ``softmax_xent`` or, for one-hot / dense targets,
  ``softmax_xent_dense``; with ``sample_weight`` either takes the staged weights and reads
  the row at the device cursor) -> ``step_fold``
  (cursor + metric accumulators in the device ``Ctrl`` block), captured once as a HIP
  graph and replayed ceil(n / batch) times: no host synchronisation per batch, one at
  the end of the call.

Plans are cached per (model, batch size); weights are re-read at the start of every call
(fp32 copy into the plan's flat buffer, one bf16 cast, the padded copies, the BN rows).
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch

from ..ops import hip as H
from ..utils import logging as dlog
from .ctrl import C_AC, C_AL, C_AN, C_CUR, C_GB, C_NS, C_ROW0, C_WRAP, WORDS, i2f
from .native_exec import PlanExec, capture
from .native_params import FlatParams
from .native_plan import (_layer_graph, _param_weights, dense_targets, layers_eligible, loss_head_ok, lower,
                          output_head, regularizers_ok)


class NativeInference:
    name = "native_infer"

    @staticmethod
    def eligible(model, device, evaluate: bool = False) -> Tuple[bool, str]:
        if torch.device(device).type != "cuda":
            return False, "not on a GPU"
        ok, why = layers_eligible(model)
        if ok and evaluate:  # (predict uses no loss: its eligibility is the layers' alone)
            ok, why = regularizers_ok(model)
            if not ok:
                return ok, why
            return loss_head_ok(model, output_head(_layer_graph(model)[0])[0])
        return ok, why

    def __init__(self, model, batch: int, device):
        # an inference plan owns no strategy, gradients or optimizer: the forward-only plan,
        # a copy of every weight it reads, and the plan's buffers and forward ops
        from ..native import require_C

        self.model, self.B, self.device = model, int(batch), torch.device(device)
        self.C = require_C()
        dev = self.device
        self.plan = lower(model, self.B, inference=True)
        # every weight the forward reads, frozen layers included (not only trainable_weights);
        # its regularizer table (evaluate): R from one reg_penalty launch per call
        self.params = FlatParams(_param_weights(model), dev)
        # BN runs from the moving statistics (bn_infer_st), the padded weight copies are made
        # once per call, an input prefix runs with flips off and crops centred
        self.ex = PlanExec(self.plan, self.params, self.C, dev, bn_fin=False, weights_static=True,
                           aug_training=False)
        self.nodes, self.in_shape, self.K, self.ctrl = self.plan.nodes, self.plan.in_shape, self.ex.K, self.ex.ctrl
        self.tail = torch.zeros(8, dtype=torch.float32, device=dev)
        self._graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}
        self._bufs: Dict[str, torch.Tensor] = {}
        self._bn = [nd for nd in self.plan.live if nd.kind == "BatchNormalization"]
        self._stream = torch.cuda.Stream(dev)

    # --- weights --------------------------------------------------------------------------
    def _refresh_weights(self):
        p = self.params
        for v in p.vars:
            p.view(v).copy_(v.value.detach().reshape(v.shape))
        H.cast_bf16(p.P, p.Pb)
        for nd in self.plan.live:
            self.ex.pad_weights(nd)
        keep = []  # moving statistics moved to the device for this call: alive until the sync
        for nd in self._bn:
            l = nd.layer
            mean, var = (w.value.detach().to(self.device, torch.float32).contiguous()
                         for w in (l.moving_mean, l.moving_variance))
            keep += [mean, var]
            H.bn_infer_st(mean, var, p.view(l.gamma), p.view(l.beta), l.epsilon, nd.attrs["bn_state"].st)
        torch.cuda.current_stream(self.device).synchronize()

    # --- the step ---------------------------------------------------------------------------
    def _infer_step(self, mode: str):
        C, B, ex = self.C, self.B, self.ex
        s = H.stream_handle()
        h, w, c = self.in_shape
        x, y = self._bufs["x"], self._bufs["y"]
        # uint8 inputs are fed as their raw values (Keras casts them), scale 1
        C.gather_batch(x.data_ptr(), int(x.dtype == torch.uint8), 1.0, y.data_ptr(), self.ctrl.data_ptr(), B,
                       h * w, c, self.plan.cin_pad, self.plan.x0.buf.data_ptr(), ex.labels.data_ptr(), s)
        ex.forward()
        if mode == "predict":
            if self.plan.head_kind == "probs":  # the model's output is the softmax of the logits
                H.softmax_store(ex.logits, self.K, self.ctrl, self._bufs["out"])
            else:
                C.logits_store(ex.logits.data_ptr(), ex.Kp, self.K, B, self.ctrl.data_ptr(),
                               self._bufs["out"].data_ptr(), s)
            C.step_fold(self.ctrl.data_ptr(), 0, s)
        elif mode.startswith("evaluate_dense"):
            # y: all-zero ids (gather_batch turns them into the 0 / -1 row validity); the
            # [n, K] target rows are read in place at the device cursor
            H.softmax_xent_dense(ex.logits, self._bufs["yd"], self.K, 1.0 / B, ex.dlogits, self.tail,
                                 label_smoothing=self._eps, labels=ex.labels, ctrl=self.ctrl, rows=ex.xent_rows,
                                 weights=self._bufs["w"] if mode.endswith("_w") else None)
            C.step_fold(self.ctrl.data_ptr(), self.tail.data_ptr(), s)
        else:
            H.softmax_xent(ex.logits, ex.labels, self.K, 1.0 / B, ex.dlogits, self.tail, ctrl=self.ctrl,
                           rows=ex.xent_rows, weights=self._bufs["w"] if mode.endswith("_w") else None)
            C.step_fold(self.ctrl.data_ptr(), self.tail.data_ptr(), s)

    def _stage(self, x, y=None, dense=False, sw=None):
        """Upload the call's inputs into (grown-only) device buffers; (re)capture happens
        only when a buffer had to be reallocated.  ``dense``: y holds [n, K] target rows,
        kept as a float buffer (the class-id buffer is then all zeros).  ``sw``: per-sample
        loss weights, float32 [n]."""
        n = len(x)
        h, w, c = self.in_shape
        x = np.asarray(x)
        u8 = x.dtype == np.uint8
        rows = x.reshape(n, h * w * c)
        if not u8:
            rows = rows.astype(np.float32, copy=False)
        self._grow("x", n, (h * w * c,), torch.uint8 if u8 else torch.float32)
        self._bufs["x"][:n].copy_(torch.from_numpy(np.ascontiguousarray(rows)), non_blocking=False)
        self._grow("y", n, (), torch.int32)
        if y is not None and dense:
            y = np.asarray(y)
            if y.ndim != 2 or y.shape[1] != self.K:
                raise ValueError(f"{type(self.model.loss).__name__} takes one-hot / dense targets of shape "
                                 f"(n, {self.K}) for this model, got y of shape {tuple(y.shape)}")
            self._grow("yd", n, (self.K,), torch.float32)
            self._bufs["yd"][:n].copy_(torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)))
            self._bufs["y"].zero_()
        elif y is not None:
            self._bufs["y"][:n].copy_(torch.from_numpy(np.asarray(y).astype(np.int32).reshape(n)))
        if sw is not None:
            sw = np.ascontiguousarray(np.asarray(sw, dtype=np.float32).reshape(-1))
            if sw.shape[0] != n:
                raise ValueError(f"sample_weight has length {sw.shape[0]} but there are {n} samples")
            self._grow("w", n, (), torch.float32)
            self._bufs["w"][:n].copy_(torch.from_numpy(sw))
        self._grow("out", n, (self.K,), torch.float32)
        return n

    def _grow(self, key, n, tail, dtype):
        """Room for n rows in the (grown-only) buffer ``key``; a reallocation drops the graphs."""
        b = self._bufs.get(key)
        if b is None or b.dtype != dtype or b.shape[0] < n:
            self._bufs[key] = torch.zeros((max(n, 1),) + tail, dtype=dtype, device=self.device)
            self._graphs.clear()

    def _ctrl_reset(self, n):
        c = torch.zeros(WORDS, dtype=torch.int32)
        c[C_NS], c[C_GB], c[C_ROW0], c[C_CUR], c[C_WRAP] = n, self.B, 0, 0, 0
        self.ctrl.copy_(c.to(self.device))
        self.tail.zero_()

    def _run(self, mode: str, n: int):
        steps = -(-n // self.B)
        dev = self.device
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(self._stream):
            self._refresh_weights()
            self._ctrl_reset(n)
            g = self._graphs.get(mode)
            if g is None:
                g = self._graphs[mode] = capture(dev, lambda: self._infer_step(mode), stream=self._stream)
            for _ in range(steps):
                g.replay()
        torch.cuda.synchronize(dev)

    # --- public ----------------------------------------------------------------------------
    @torch.no_grad()
    def predict(self, x) -> np.ndarray:
        n = self._stage(x)
        if n == 0:
            return np.zeros((0, self.K), dtype=np.float32)
        self._run("predict", n)
        return self._bufs["out"][:n].cpu().numpy()

    @torch.no_grad()
    def evaluate_sums(self, x, y, sample_weight=None) -> Tuple[float, float, float]:
        """(sum of per-sample loss, number of samples, number correct) over (x, y); with
        ``sample_weight`` (float32 [n]) the sum of w_i * loss_i, the two counts unweighted."""
        dense = dense_targets(self.model)
        n = self._stage(x, y, dense=dense, sw=sample_weight)
        if n == 0:
            return 0.0, 0.0, 0.0
        if dense:
            eps = float(self.model.loss.label_smoothing or 0.0)
            if eps != getattr(self, "_eps", None):  # a kernel argument of the captured step
                self._eps = eps
                self._graphs.pop("evaluate_dense", None)
                self._graphs.pop("evaluate_dense_w", None)
        self._run(("evaluate_dense" if dense else "evaluate") + ("_w" if sample_weight is not None else ""), n)
        c = self.ctrl.cpu().tolist()
        loss, cnt = i2f(c[C_AL]), i2f(c[C_AN])
        p = self.params
        if p.reg_tab is not None:
            # the weights are static during the call: every row's loss gains the same R
            H.reg_penalty(p.P, p.reg_tab, p.reg_scratch)
            torch.cuda.synchronize(self.device)
            loss += float(p.reg_scratch[-1]) * cnt
        return loss, cnt, i2f(c[C_AC])


def plan_for(model, batch: int, device, evaluate: bool = False):
    """The cached inference plan of ``model`` at ``batch`` (None when ineligible)."""
    ok, why = NativeInference.eligible(model, device, evaluate)
    if not ok:
        dlog.warning("native inference unavailable (%s): %s runs on PyTorch ops", why,
                     "evaluate" if evaluate else "predict")
        return None
    cache = model.__dict__.setdefault("_infer_plans", {})
    key = (int(batch), str(device))
    p = cache.get(key)
    if p is None:
        p = NativeInference(model, batch, device)
        cache[key] = p
    return p
