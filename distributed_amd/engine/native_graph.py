"""Native graph engine: any supported Keras model lowered to a static plan of HIP kernel
launches (no autograd, no per-op Python on the hot path), captured as a HIP graph.

This is the generic-model counterpart of the fused MNIST trainer (fused_convnet.py),
used for ResNet-style networks (BASELINE.json config 4) and any
other model built from the supported layers.  What happens per step (one rank):

    gather_batch (device cursor, uint8/fp32 -> bf16 NHWC, channel padding)
    augment:  a ZeroPadding2D / RandomCrop / RandomFlip chain at the model input, one launch
              (csrc/kernels/augment.hip; only for models that begin with such a chain)
    forward:  implicit-GEMM MFMA convs / dense (csrc/kernels/gemm.hip) with bias / ReLU /
              BatchNorm-statistics epilogues, fused BN(+residual)(+ReLU) apply, pooling
    loss:     softmax cross-entropy + accuracy -> dlogits and the metric tail of G (with
              sample / class weights: each row's gradient and loss times the weight of its
              sample, read from the epoch-ordered weights at the device cursor)
    backward: reverse plan: BN backward (3 passes), pooling backward, dgrad GEMMs
              (residual fan-in accumulated in the GEMM epilogue), wgrad GEMMs accumulated
              with fp32 atomics straight into the flat gradient buffer G (split-K)
    all-reduce G (RCCL, in the graph) -> flat SGD (+momentum) that also refreshes the
              bf16 weight shadow and advances the device cursor / epoch accumulators.

The engine is four parts: the device-free plan and its fusion rules (native_plan.py), the
flat parameter / gradient / slot buffers (native_params.py), the plan's buffers and forward
ops (native_exec.py: memory is planned once, so the captured graph replays with no
allocation) and the gradient buckets with their all-reduce transport (native_buckets.py).
This module holds what trains over them: the Ctrl block and hyper-parameters, data binding,
the step (loss, backward ops, optimizer) and the driver.
"""
from __future__ import annotations

import weakref
from contextlib import contextmanager

import numpy as np
import torch

from ..ops import hip as H
from ..utils import env
from ..utils import logging as dlog
from .base import Engine
from .ctrl import C_GB, C_IT, C_LR, C_NS, C_ROW0, epoch_metrics, epoch_start_words, f2i, hparam_words, rmw
from .data import DataFeed
from .native_buckets import BucketReducer
from .native_exec import PlanExec, capture
from .native_params import FlatParams
from .native_plan import (T, _act_name, _layer_graph, _opt_kernel_slots, _param_weights, _schedule_of, clipping_ok,
                          dense_targets, layers_eligible, loss_head_ok, lower, output_head, regularizers_ok,
                          schedule_ok)

class NativeGraphEngine(Engine):
    name = "native_graph"
    layers_eligible = staticmethod(layers_eligible)

    @staticmethod
    def eligible(model, strategy):
        from ..keras import losses, optimizers

        if strategy.device.type != "cuda":
            return False, "not on a GPU"
        if type(model.optimizer) not in (optimizers.SGD, optimizers.Adam, optimizers.RMSprop):
            return False, f"optimizer {type(model.optimizer).__name__}"
        if not isinstance(model.loss, (losses.SparseCategoricalCrossentropy, losses.CategoricalCrossentropy)):
            return False, "loss"
        # the training plan keeps one flat buffer of trainable weights: a frozen kernel /
        # bias / gamma / beta (layer.trainable = False) trains on the generic path
        trainable = {id(w) for w in model.trainable_weights}
        if any(id(w) not in trainable for w in _param_weights(model)):
            return False, "frozen layer weights"
        for check in (layers_eligible, regularizers_ok, clipping_ok, schedule_ok):
            ok, why = check(model)
            if not ok:
                return ok, why
        return loss_head_ok(model, output_head(_layer_graph(model)[0])[0])

    # ------------------------------------------------------------------------------------
    def __init__(self, model, strategy, per_replica_batch, global_batch):
        super().__init__(model, strategy, per_replica_batch, global_batch)
        from ..native import require_C

        self.C = require_C()
        dev, opt = self.device, model.optimizer
        self.B = per_replica_batch
        # params: weights, gradients and optimizer state on the device, flat
        self._init_params()
        p = self.params
        # plan -> its buffers and forward ops
        self.plan = pl = lower(model, self.B, rank=self.rank)
        self.ex = ex = PlanExec(pl, p, self.C, dev, bn_fin=True, weights_static=False, aug_training=True)
        self.nodes, self.x0, self.in_shape, self.cin_pad = pl.nodes, pl.x0, pl.in_shape, pl.cin_pad
        self.head_kind, self.head_node, self.K = pl.head_kind, pl.head_node, ex.K
        self.labels, self.logits, self.dlogits, self.gemm_ws = ex.labels, ex.logits, ex.dlogits, ex.gemm_ws
        # target kind of the loss launch: class ids (softmax_xent) or dense [n, K] rows
        # (softmax_xent_dense, with the loss' label smoothing)
        self.dense_y = dense_targets(model)
        self.label_smoothing = float(getattr(model.loss, "label_smoothing", 0.0) or 0.0) if self.dense_y else 0.0
        # buckets: the gradient all-reduce transport (a norm clip needs the whole gradient)
        self.reducer = r = BucketReducer(strategy, self.C, dev, p, pl,
                                         norm_clip=self.clip_mode if self.clip_plan is not None else None)
        self._buckets, self.bucket_comms, self.bucket_opt = r.buckets, r.bucket_comms, r.bucket_opt
        self.peer, self.peers, self.allreduce_kind = r.peer, r.peers, r.allreduce_kind
        self.host_collective, self.grad_bf16 = r.host_collective, r.grad_bf16
        self.use_graph = env.get_bool("DAMD_GRAPH", True) and not self.host_collective
        # convolution weight gradients on a side stream (DAMD_WGRAD_STREAM): a conv's
        # weight gradient and its backprop-input read the same dy and are independent, so
        # the weight-gradient kernel (+ its split-K reduce) runs beside the backprop-input /
        # BatchNorm-backward chain of the main stream (own workspace); joined before the
        # optimizer, and every bucket all-reduce waits for it
        self._wgrad_stream = r.wgrad_stream
        self.gemm_ws_w = torch.zeros_like(self.gemm_ws) if self._wgrad_stream is not None else None
        self._wgrad_side_minc = env.get_int("DAMD_WGRAD_STREAM_MINC", 0)  # convs with fewer outputs stay inline
        # ctrl
        self.ctrl = ex.ctrl
        self._ctrl_write({C_IT: int(opt.iterations), C_ROW0: self.rank * self.per_replica, C_GB: self.global_batch,
                          **self._hparam_words()})
        opt._iter_source = self._iterations
        self.graph = None
        self._phase_events = None  # phase_times(): (name, event) marks of an eager step
        self.feed = None
        torch.cuda.synchronize(dev)
        dlog.info("native graph engine: %d nodes, %d params, %.1f MB planned activations", len(self.nodes),
                  self.nparam, ex.act_bytes / 2**20)

    def _init_params(self):
        model, dev, opt = self.model, self.device, self.model.optimizer
        # flat fp32 masters P (Keras trainable-weight order), bf16 shadow Pb, gradients G, and
        # the optimizer slots (SGD momentum; Adam m, v, vhat; RMSprop rms, momentum, mean
        # gradient -- S0..S2 of the opt_step kernel) in the same padded layout
        self.opt_kind, self.slot_kernel_names = _opt_kernel_slots(opt)
        self.params = p = FlatParams(model.trainable_weights, dev, train=True, slots=self.slot_kernel_names)
        self.vars, self.sizes, self.offsets, self.nparam = p.vars, p.sizes, p.offsets, p.n
        self.P, self.Pb, self.G, self.S, self.views = p.P, p.Pb, p.G, p.S, p.views
        self.reg_tab, self.reg_scratch = p.reg_tab, p.reg_scratch
        self._slot_dummy = torch.zeros(8, dtype=torch.float32, device=dev)
        self.V = self.S.get("momentum", self._slot_dummy)
        self._own_variables(self.vars)
        # gradient clipping (keras/optimizers.py), constants of the captured step.  clipvalue
        # lives inside opt_step; the two norm modes run one grad_norm launch over the whole
        # all-reduced G before the single opt_step: tables, scratch and scales built here
        self.clip_mode, self.clip_c = opt.clipping()
        self.clip_plan = None
        if self.clip_mode in ("clipnorm", "global_clipnorm"):
            co = {r[0]: (r[2], r[3]) for r in p.reg_rows}
            self.clip_plan = H.clip_plan([(o, sz) + co.get(o, (0.0, 0.0)) for o, sz in zip(p.offsets, p.sizes)], p.n,
                                         dev, per_variable=self.clip_mode == "clipnorm")
        # learning-rate schedule (keras/schedules.py): opt_step's descriptor, a constant of the
        # captured step built once (None: a plain rate, read from ctrl).  The optimizer tells
        # the engine when a schedule is assigned or removed (lr_changed).
        self._build_lr_table()
        opt._lr_listener = weakref.WeakMethod(self.lr_changed)
        # non-trainable (BN moving statistics) live on the device as fp32
        for w in model.non_trainable_weights:
            if w.value.device != dev:
                w._rebind(torch.zeros(w.shape, dtype=torch.float32, device=dev))
        self._load_momentum()
        if self.world > 1:
            comm = self.strategy.communicator
            comm.broadcast_(self.P, 0)
            for w in model.non_trainable_weights:
                comm.broadcast_(w.value, 0)
        H.cast_bf16(self.P, self.Pb)

    # --- the plan ---------------------------------------------------------------------------
    @staticmethod
    def plan_only(model, batch: int):
        """The fused plan of ``model`` at per-replica batch ``batch`` without touching a
        device (planner inspection / CPU tests)."""
        return lower(model, batch)

    def describe_plan(self) -> dict:
        return self.plan.describe()

    def graph_nodes(self):
        """Structure of one captured step (tests): [(node type, kernel name, [dependency
        indices])] of a fresh capture whose hipGraph is kept (C.graph_nodes)."""
        torch.cuda.synchronize(self.device)
        g = capture(self.device, self._step_body, keep_graph=True)
        torch.cuda.synchronize(self.device)
        nodes = self.C.graph_nodes(g.raw_cuda_graph())
        del g
        return nodes

    # --- gradient write protocol ----------------------------------------------------------
    @contextmanager
    def _grad_into(self, t: T):
        """The buffer a producer of t's gradient writes: None when t takes no gradient, the
        gradient itself for its first writer, else scratch that is added into it on exit."""
        r = t.root()
        if not r.needs_grad:
            yield None
        elif not r.written:
            r.written = True
            yield r.grad
        else:
            tmp = self.ex.scratch[: r.grad.numel()].view(r.grad.shape)
            yield tmp
            H.add_bf16(r.grad, tmp, r.grad)

    # --- hyper-parameters / ctrl -------------------------------------------------------------
    def _build_lr_table(self):
        self.lr_sched = _schedule_of(self.model.optimizer)
        self.lr_tab = H.lr_table(self.lr_sched, self.device) if self.lr_sched is not None else None

    def _host_lr(self):
        """The rate for ctrl's lr: the number, or the schedule at the current iterations
        (what the next step's kernel will compute and store there itself)."""
        opt = self.model.optimizer
        if self.lr_sched is not None:
            return float(self.lr_sched(int(opt.iterations)))
        return opt.learning_rate

    def _hparam_words(self):
        opt = self.model.optimizer
        return hparam_words(self._host_lr(), getattr(opt, "momentum", 0.0), getattr(opt, "nesterov", False))

    def _ctrl_write(self, updates):
        torch.cuda.synchronize(self.device)
        rmw(self.ctrl, updates)
        torch.cuda.synchronize(self.device)

    def _iterations(self):
        torch.cuda.synchronize(self.device)
        return int(self.ctrl[C_IT].item())

    def lr_changed(self):
        sched = _schedule_of(self.model.optimizer)
        if sched is not self.lr_sched:
            # a schedule came, went or was replaced: the descriptor is baked into the captured
            # step's optimizer launches
            torch.cuda.synchronize(self.device)
            self.graph = None
            if not schedule_ok(self.model)[0]:
                # no native form: the next fit selects an engine again, and the fallback
                # warning (or DAMD_STRICT_NATIVE's error) says why
                self.model._engine_key = None
                return
            self._build_lr_table()
        self._ctrl_write({C_LR: f2i(self._host_lr())})

    def _load_momentum(self):
        # optimizer slots are dense over the unpadded weights (Keras order)
        opt = self.model.optimizer
        tot = int(sum(self.sizes))
        for nm, buf in self.S.items():
            if nm in opt.slots and opt.slots[nm].numel() == tot:
                src = opt.slots[nm].to(self.device)
                o = 0
                for sz, off in zip(self.sizes, self.offsets):
                    buf[off:off + sz].copy_(src[o:o + sz])
                    o += sz

    def reload_optimizer_state(self):
        torch.cuda.synchronize(self.device)
        self._load_momentum()
        it = self._host_iterations()
        H.cast_bf16(self.P, self.Pb)
        self._ctrl_write({C_IT: it})

    # --- data -------------------------------------------------------------------------------
    def bind(self, x, y, w=None):
        x = np.asarray(x)
        sw = w  # per-sample loss weights (float32 [n]) or None
        h, w, c = self.in_shape
        if tuple(x.shape[1:]) not in ((h, w, c),) and not (c == 1 and tuple(x.shape[1:]) == (h, w)):
            raise ValueError(f"native graph engine expects inputs of shape {(h, w, c)}, got {x.shape[1:]}")
        if self.dense_y:
            ys = np.shape(y)
            if len(ys) != 2 or ys[1] != self.K:
                raise ValueError(f"{type(self.model.loss).__name__} takes one-hot / dense targets of shape "
                                 f"(n, {self.K}) for this model, got y of shape {tuple(ys)}"
                                 " (to_categorical(y), or the sparse loss for class ids)")
        if self.feed is None or not self.feed.built_from(x, y, sw):
            torch.cuda.synchronize(self.device)
            self.feed = DataFeed(x, y, self.device, flatten=True, allow_u8=env.get_bool("DAMD_X_U8", True), w=sw)
            if self.dense_y and (self.feed.y.dtype != torch.float32 or tuple(self.feed.y.shape) !=
                                 (self.feed.n, self.K)):
                raise ValueError(f"dense targets must be (n, {self.K}) numbers, got {tuple(self.feed.y.shape)}")
            # (the weights in epoch order beside x_ep / y_ep: the loss launch reads the row at
            # the device cursor; None: the unweighted launch)
            self.feed.alloc_epoch()
            self.y_zero = torch.zeros(self.feed.n, dtype=torch.int32, device=self.device) if self.dense_y else None
            self.graph = None  # data pointers changed
            self._ctrl_write({C_NS: self.feed.n})
        return self.feed

    def start_epoch(self, epoch, shuffle, wrap_steps: int = 0):
        torch.cuda.synchronize(self.device)
        self.feed.set_epoch(epoch, shuffle, self.shuffle_seed)
        self.feed.fill_epoch()
        self._ctrl_write({**epoch_start_words(wrap_steps), **self._hparam_words()})

    # --- the step ----------------------------------------------------------------------------
    def _mark(self, name):
        ev = self._phase_events
        if ev is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            ev.append((name, e))

    def _step_body(self):
        C, B, ex = self.C, self.B, self.ex
        s = H.stream_handle()
        self._mark("start")
        h, w, c = self.in_shape
        # the step's first launch also clears the gradient buffer (and the BN statistics
        # accumulators): no memset launch in the step; and it refreshes the first padded
        # conv's bf16 weight copy (PlanExec.pad_folded)
        acc = ex.bn_acc
        live = self.plan.live
        job = ex.pad_job(ex.pad_folded) if ex.pad_folded is not None else None
        # (dense targets: gather_batch gets an all-zero label array, so self.labels still
        # carries 0 for a real row and -1 for one past the end of the data)
        feed = self.feed
        y_ids = self.y_zero if self.dense_y else feed.y_ep
        C.gather_batch(feed.x_ep.data_ptr(), int(feed.x_u8), 255.0, y_ids.data_ptr(), self.ctrl.data_ptr(),
                       B, h * w, c, self.cin_pad, self.x0.buf.data_ptr(), self.labels.data_ptr(), s,
                       zero=self.G.data_ptr(), zero_bytes=self.G.numel() * 4,
                       zero2=acc.data_ptr() if acc is not None else 0, zero2_bytes=acc.numel() * 8 if acc is not None else 0,
                       pc_src=job[0].data_ptr() if job else 0, pc_dst=job[1].data_ptr() if job else 0,
                       pc_dims=list(job[2:]) if job else [])
        ex.forward()
        last = self.head_node
        # (the logits layer's bias gradient out of the loss launch: PlanExec's bias_folded)
        bias_grad = self.params.gview(last.layer.bias) if last.attrs["bias_folded"] else None
        if self.dense_y:
            # one-hot / soft targets: the kernel reads the epoch-ordered [n, K] rows in place
            # at the device cursor (self.labels: the 0 / -1 row validity gather_batch wrote)
            H.softmax_xent_dense(self.logits, feed.y_ep, self.K, 1.0 / self.global_batch, self.dlogits,
                                 self.G[self.nparam:], label_smoothing=self.label_smoothing, labels=self.labels,
                                 ctrl=self.ctrl, rows=ex.xent_rows, bias_grad=bias_grad, weights=feed.w_ep)
        else:
            H.softmax_xent(self.logits, self.labels, self.K, 1.0 / self.global_batch, self.dlogits,
                           self.G[self.nparam:], ctrl=self.ctrl, rows=ex.xent_rows, bias_grad=bias_grad,
                           weights=feed.w_ep)
        if self.reg_tab is not None:
            # loss sum += R(w) per valid local row (tail[2]), before the tail leaves with
            # bucket 0's all-reduce: the SUM over replicas yields R * (global rows)
            H.reg_penalty(self.P, self.reg_tab, self.reg_scratch, tail=self.G[self.nparam:])
        self._mark("forward")
        for t in self.plan.all_tensors():
            t.root().written = False
        self.reducer.begin()
        for nd in reversed(live):
            getattr(self, "_bwd_" + nd.kind)(nd)
            self.reducer.progress(nd, self._optimizer_step)
        if self._wgrad_stream is not None:
            torch.cuda.current_stream(self.device).wait_stream(self._wgrad_stream)
        self._mark("backward")
        self.reducer.progress(None, self._optimizer_step, final=True)
        self._mark("allreduce")  # the part of the all-reduce not hidden behind backward
        if not self.host_collective and not self.bucket_opt:
            self._optimizer_step()
        self._mark("optimizer")

    def _optimizer_step(self, b=None):
        """The optimizer update of every parameter (b None), or of bucket b's range only --
        the bucket whose range holds the metric tail also does the step's bookkeeping."""
        opt = self.model.optimizer
        ptr = [self.S[nm].data_ptr() if nm else self._slot_dummy.data_ptr() for nm in self.slot_kernel_names]
        if self.opt_kind == 1:
            args = (float(opt.beta_1), float(opt.beta_2), float(opt.epsilon), 0.0, 0.0, int(opt.amsgrad))
        elif self.opt_kind == 2:
            args = (0.0, 0.0, float(opt.epsilon), float(opt.rho), float(opt.momentum), int(opt.centered))
        else:
            args = (0.0, 0.0, 0.0, 0.0, float(opt.momentum), int(opt.nesterov))
        lo, hi, book = 0, self.nparam, 1
        if b is not None:
            lo, hi = b["lo"], min(b["hi"], self.nparam)
            book = int(b["hi"] > self.nparam)
        # (a slot pointer of an unused slot is the dummy: offset, never dereferenced)
        o4 = 4 * lo
        tab, clip = self.reg_tab, {}
        if self.clip_mode is not None:
            clip = dict(clip=H.CLIP_KINDS[self.clip_mode], clipc=self.clip_c)
        if self.clip_plan is not None:
            # the norm(s) of the whole all-reduced gradient (+ dR/dw) first: one launch on this
            # stream, behind every bucket's all-reduce, then the single update
            assert b is None, "norm clipping updates every parameter in one launch"
            H.grad_norm(self.G, self.clip_plan, self.clip_c, P=self.P if self.clip_plan.regularized else None)
            clip["scales"] = self.clip_plan.scales.data_ptr()
            if self.clip_plan.per_variable:
                tab = self.clip_plan.vt  # every variable: the row index is the scale index
        self.C.opt_step(self.P.data_ptr() + o4, self.G.data_ptr() + o4, ptr[0] + o4, ptr[1] + o4, ptr[2] + o4,
                        self.Pb.data_ptr() + 2 * lo, max(hi - lo, 0), self.ctrl.data_ptr(),
                        self.G[self.nparam:].data_ptr(), self.opt_kind, *args, H.stream_handle(), book=book,
                        reg=tab.data_ptr() if tab is not None else 0,
                        nreg=tab.shape[0] if tab is not None else 0, lo=lo,
                        lr=self.lr_tab.data_ptr() if self.lr_tab is not None else 0, **clip)

    # --- backward ops -----------------------------------------------------------------------
    def _bwd_Augment(self, nd):
        pass  # the input has no gradient

    def _bwd_Conv2D(self, nd):
        l = nd.layer
        xt = nd.inputs[0].root()
        y = nd.out.root()
        dy = y.grad
        if "dz" in nd.attrs:
            self._act_bwd(nd, dy, y.buf, nd.attrs["dz"])
            dy = nd.attrs["dz"]
        side = self._wgrad_stream
        if side is not None and l.kernel.shape[-1] >= self._wgrad_side_minc:
            side.wait_stream(torch.cuda.current_stream(self.device))  # dy and x are final
            with torch.cuda.stream(side):
                self._conv_wgrad(nd, xt, dy, self.gemm_ws_w)
        else:
            self._conv_wgrad(nd, xt, dy, self.gemm_ws)
        if xt.needs_grad:
            wb = nd.attrs.get("w_pad", self.params.bview(l.kernel))
            acc = xt.written
            xt.written = True
            # first (only) writer of a BN -> ReLU output gradient: the BN-backward partials come
            # out of this launch's epilogue
            bn = nd.attrs.get("bnred")
            bnred = None
            if bn is not None and not acc:
                bnred = (bn.inputs[0].root().buf, bn.attrs["bn_state"].st, bn.attrs["bn_state"].dgrad)
            fused = H.conv_dgrad(dy, wb, xt.grad, l.strides, l.padding, accumulate=acc, workspace=self.gemm_ws,
                                 bnred=bnred)
            if bn is not None:
                bn.attrs["bn_state"].dgrad_fused = bnred is not None and fused

    def _conv_wgrad(self, nd, xt, dy, ws):
        """Bias and weight gradient of conv node nd (current stream, workspace ws)."""
        l = nd.layer
        if l.use_bias:
            H.colsum(dy, self.params.gview(l.bias), workspace=ws)
        if nd.attrs.get("stem4"):
            kh, kw, cin, cout = l.kernel.shape
            dwp = nd.attrs["dw_pad"]
            # split-K: the reduce adds straight into the gradient view (0 + sum, as
            # unpad_add(reduce) did: the same bits); one split: the atomic GEMM into dw_pad
            if not H.conv_wgrad_stem4(xt.buf, dy, dwp, kh, l.strides, l.padding, workspace=ws, accumulate=False,
                                      dw=self.params.gview(l.kernel)):
                H.unpad_add(dwp, kh, kw, cin * cout, 8, 4 * cout, self.params.gview(l.kernel))
        elif "dw_pad" in nd.attrs:
            dwp = nd.attrs["dw_pad"]
            H.conv_wgrad(xt.buf, dy, dwp, l.strides, l.padding, workspace=ws, accumulate=False)
            kh, kw, cin, cout = l.kernel.shape
            H.unpad_add(dwp, kh * kw, cin, cout, nd.attrs["cin_pad"], cout, self.params.gview(l.kernel))
        else:
            H.conv_wgrad(xt.buf, dy, self.params.gview(l.kernel), l.strides, l.padding, workspace=ws)

    def _bwd_DepthwiseConv2D(self, nd):
        l = nd.layer
        xt = nd.inputs[0].root()
        y = nd.out.root()
        dy, g = y.grad, nd.attrs["geo"]
        if "dz" in nd.attrs:
            self._act_bwd(nd, dy, y.buf, nd.attrs["dz"])
            dy = nd.attrs["dz"]
        if l.use_bias:
            H.colsum(dy, self.params.gview(l.bias), workspace=self.gemm_ws)
        H.dwconv_wgrad(xt.buf, dy, g, self.params.gview(l.depthwise_kernel), workspace=self.gemm_ws)
        with self._grad_into(xt) as dx:  # (a second writer: scratch + add_bf16)
            if dx is not None:
                H.dwconv_dgrad(dy, self.params.bview(l.depthwise_kernel), g, dx)

    def _bn_backward(self, bn, dy, ymask, relu, dz_out=None, mask_from_x=False):
        """BatchNorm backward of node ``bn`` for upstream gradient dy (masked by
        [ymask > 0] when relu); dgamma/dbeta into the gradient sinks, dx into the input's
        gradient; optionally also writes the masked dy to dz_out.  ``mask_from_x``: the
        output is bn_apply(x, relu) with no residual, so the kernels recompute the ReLU
        mask from x (already read) instead of reading the stored output."""
        x, b = bn.inputs[0].root(), bn.attrs["bn_state"]
        mode = (2 if mask_from_x else 1) if relu else 0
        # the sums already written by the consuming conv's backprop-input epilogue?
        fused = b.dgrad_fused and mode == 2 and dz_out is None
        # (dx is None only for a BatchNorm on the plan's input, which has no conv statistics and so
        # carries partials: an accumulator's apply never gets a null dx)
        with self._grad_into(x) as dx:
            H.bn_bwd(dy, ymask if relu else None, mode, x.buf, b.st, co=b.co, dx=dx,
                     dgamma=self.params.gview(bn.layer.gamma), dbeta=self.params.gview(bn.layer.beta),
                     dz_out=dz_out if relu else None, reduce=not fused, **b.carry(b.dgrad if fused else None))

    def _bwd_BatchNormalization(self, nd):
        if nd.attrs.get("stats_only") or nd.attrs.get("pool") is not None:
            return  # handled by the fused Add / MaxPool
        y = nd.out.root()
        self._bn_backward(nd, y.grad, y.buf, bool(nd.attrs.get("relu")),
                          mask_from_x=env.get_bool("DAMD_BN_MASK_FROM_X", True))

    def _act_bwd(self, nd, dy, y, dx):
        an = _act_name(nd.layer) if nd.kind != "ReLU" else "relu"
        if an == "relu" and dy.numel() % 8 == 0:
            H.relu_bwd(dy, y, dx)
        else:
            H.act_bwd(dy, y, dx, an)

    def _bwd_Activation(self, nd):
        y = nd.out.root()
        with self._grad_into(nd.inputs[0]) as dx:
            if dx is not None:
                self._act_bwd(nd, y.grad, y.buf, dx)

    def _bwd_Dropout(self, nd):
        with self._grad_into(nd.inputs[0]) as dx:
            if dx is not None:
                # the same counter-hash mask and scale as the forward (same seed, same step t)
                H.dropout(nd.out.root().grad, dx, self.ctrl, nd.attrs["seed"], nd.layer.rate)

    def _bwd_AveragePooling2D(self, nd):
        l = nd.layer
        with self._grad_into(nd.inputs[0]) as dx:
            if dx is not None:
                H.avgpool_bwd(nd.out.root().grad, dx, l.pool_size, l.strides, l.padding)

    _bwd_ReLU = _bwd_Activation

    def _bwd_Add(self, nd):
        out = nd.out.root()
        fused = nd.attrs.get("fused")
        if fused is None:
            for x in nd.inputs:
                with self._grad_into(x) as dx:
                    if dx is not None:
                        dx.copy_(out.grad)
            return
        main, (mode, other) = fused
        relu = bool(nd.attrs.get("relu"))
        dy = out.grad
        if mode == "raw":
            # the residual input's gradient is the (masked) dy itself
            with self._grad_into(other) as dz:
                if relu:
                    self._bn_backward(main, dy, out.buf, True, dz_out=dz)
                else:
                    if dz is not None:
                        dz.copy_(dy)
                    self._bn_backward(main, dy, out.buf, False)
        else:
            # both BN backwards mask dy by [out > 0] themselves (no separate ReLU-backward pass)
            if not self._bn_backward_dual(main, other, dy, out.buf, relu):
                self._bn_backward(main, dy, out.buf, relu)
                self._bn_backward(other, dy, out.buf, relu)

    def _bn_backward_dual(self, b1, b2, dy, ymask, relu):
        """Both BatchNorms of relu(BN(x) + BN(xd)) in one reduce and one apply launch
        (H.bn_bwd_fin_dual) when both finalize in their consumers and own their inputs'
        gradients (DAMD_BN_DUAL=0: four launches)."""
        if not env.get_bool("DAMD_BN_DUAL", True):
            return False
        xs = [b.inputs[0].root() for b in (b1, b2)]
        if (any(b.attrs["bn_state"].carrier != "acc" or b.attrs["bn_state"].dgrad_fused for b in (b1, b2))
                or xs[0] is xs[1] or any(x.written or not x.needs_grad for x in xs)
                or xs[0].shape != xs[1].shape or xs[0].shape[-1] % 8 or 256 % (xs[0].shape[-1] // 8)):
            return False
        with self._grad_into(xs[0]) as dx1, self._grad_into(xs[1]) as dx2:  # first writers (checked above)
            args = [{"x": x.buf, "st": b.attrs["bn_state"].st, "acc": b.attrs["bn_state"].bwd,
                     "co": b.attrs["bn_state"].co, "dx": dx,
                     "dgamma": self.params.gview(b.layer.gamma), "dbeta": self.params.gview(b.layer.beta)}
                    for b, x, dx in zip((b1, b2), xs, (dx1, dx2))]
            H.bn_bwd_fin_dual(dy, ymask if relu else None, 1 if relu else 0, args)
        return True

    def _bwd_MaxPooling2D(self, nd):
        l = nd.layer
        bn = nd.attrs.get("bn")
        if bn is not None:  # the whole BN(+ReLU) backward of the fused stem
            x, b = bn.inputs[0].root(), bn.attrs["bn_state"]
            with self._grad_into(x) as dx:
                H.pool_bn_bwd(nd.out.root().grad, nd.attrs["arg"], x.buf, b.st, co=b.co, dx=dx, pool=l.pool_size,
                              strides=l.strides, padding=l.padding, dgamma=self.params.gview(bn.layer.gamma),
                              dbeta=self.params.gview(bn.layer.beta), **b.carry())
            return
        with self._grad_into(nd.inputs[0]) as dx:
            if dx is not None:
                H.maxpool_bwd(nd.out.root().grad, nd.attrs["arg"], dx, l.pool_size, l.strides, l.padding)

    def _bwd_GlobalAveragePooling2D(self, nd):
        with self._grad_into(nd.inputs[0]) as dx:
            if dx is not None:
                H.gap_bwd(nd.out.root().grad, dx)

    def _bwd_Dense(self, nd):
        l = nd.layer
        xt = nd.inputs[0].root()
        x2 = xt.buf.view(xt.buf.shape[0], -1)
        dy = self.dlogits if nd.attrs.get("logits") else nd.out.root().grad
        if "dz" in nd.attrs:
            y = nd.out.root()
            self._act_bwd(nd, dy, y.buf, nd.attrs["dz"])
            dy = nd.attrs["dz"]
        units = l.units
        if l.use_bias and not nd.attrs.get("bias_folded"):
            H.colsum(dy, self.params.gview(l.bias), workspace=self.gemm_ws, M=dy.shape[0], N=units, ld=dy.shape[1])
        if "dw_pad" in nd.attrs:
            dwp = nd.attrs["dw_pad"]
            H.dense_wgrad(x2, dy, dwp, workspace=self.gemm_ws, accumulate=False)
            kin = l.kernel.shape[0]
            H.unpad_add(dwp, 1, kin, units, kin, dwp.shape[1], self.params.gview(l.kernel))
        else:
            H.dense_wgrad(x2, dy, self.params.gview(l.kernel), workspace=self.gemm_ws)
        if xt.needs_grad:
            wb = nd.attrs.get("w_pad", self.params.bview(l.kernel))
            acc = xt.written
            xt.written = True
            H.dense_dgrad(dy, wb, xt.grad.view(xt.grad.shape[0], -1), accumulate=acc, workspace=self.gemm_ws)

    # --- driver ---------------------------------------------------------------------------------
    def run(self, n_steps):
        if self.host_collective:
            for _ in range(n_steps):
                self._step_body()
                torch.cuda.synchronize(self.device)
                self.strategy.communicator.allreduce_(self.G, "sum")
                self._optimizer_step()
            return
        if not self.use_graph:
            for _ in range(n_steps):
                self._step_body()
            return
        done = 0
        if self.graph is None:
            # eager first step (also validates the plan), then capture
            self._step_body()
            done = 1
            if n_steps > 1:
                self._capture_safe()
                # capture does not execute; replay below
        for _ in range(n_steps - done):
            if self.graph is None:
                self._capture_safe()
            self.graph.replay()

    def phase_times(self, n_steps: int) -> dict:
        """Per-phase device time of eager steps: forward (incl. loss), backward, the exposed
        all-reduce (what is left after the buckets overlapped backward), optimizer."""
        if self.host_collective:
            return super().phase_times(n_steps)
        self.sync()
        acc = {}
        for _ in range(n_steps):
            self._phase_events = []
            self._step_body()
            evs, self._phase_events = self._phase_events, None
            torch.cuda.synchronize(self.device)
            for (_, a), (name, b) in zip(evs, evs[1:]):
                acc[name] = acc.get(name, 0.0) + a.elapsed_time(b)
        out = {k: v / max(n_steps, 1) for k, v in acc.items()}
        out["step"] = sum(out.values())
        out["allreduce_kind"] = self.allreduce_kind
        return out

    def prepare(self, n_steps):
        if self.use_graph and not self.host_collective and self.graph is None and n_steps > 0:
            self._capture_safe()

    def _capture_safe(self):
        # capturing would run allocator/stream ops; make sure no work is pending
        torch.cuda.synchronize(self.device)
        g = capture(self.device, self._step_body)
        torch.cuda.synchronize(self.device)
        self.graph = g

    def metrics(self):
        self.sync()
        return epoch_metrics(self.ctrl.cpu().tolist(), [m.name for m in self.model.compiled_metrics])

    def finish(self):
        torch.cuda.synchronize(self.device)
        opt = self.model.optimizer
        if self.S:
            tot = int(sum(self.sizes))
            opt.ensure_slots(tot, self.device)
            for nm, buf in self.S.items():
                o = 0
                for sz, off in zip(self.sizes, self.offsets):
                    opt.slots[nm][o:o + sz].copy_(buf[off:off + sz])
                    o += sz

    def sync(self):
        torch.cuda.synchronize(self.device)
        self.reducer.check_peer()  # never hand out weights built from a timed-out (partial) reduction

    def after_external_write(self):
        # the forward/backward GEMMs read the bf16 shadow Pb: re-derive it from the
        # overwritten fp32 masters before the next step
        H.cast_bf16(self.P, self.Pb)
        torch.cuda.synchronize(self.device)
