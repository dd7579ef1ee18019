"""A lowered plan (native_plan.py) on the device: its buffers, planned once (bf16 activations +
gradients for every tensor -- small next to 288 GB of HBM) so that a captured step replays
with no allocation, and its forward ops; :func:`capture` records a step as a HIP graph."""
from __future__ import annotations

import gc
from dataclasses import dataclass

import numpy as np
import torch

from ..ops import hip as H
from ..utils import env
from .native_plan import T, _act_name, _pad8


def capture(device, fn, *, stream=None, keep_graph=False):
    """``fn()`` captured as a HIP graph (not executed), on ``stream`` or on a fresh side
    stream ordered behind and before the current one.  The caller synchronises around it:
    capturing runs allocator / stream ops, so no work may be pending."""
    g = torch.cuda.CUDAGraph(keep_graph=True) if keep_graph else torch.cuda.CUDAGraph()
    s = stream
    if s is None:
        s = torch.cuda.Stream(device)
        s.wait_stream(torch.cuda.current_stream(device))
    # no garbage collection inside the capture: a finalizer that synchronises or frees
    # device resources (an old engine's communicator, graph, events) is illegal while a
    # stream captures and aborts the process (seen on the GPU tier)
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                fn()
    finally:
        if was:
            gc.enable()
    if stream is None:
        torch.cuda.current_stream(device).wait_stream(s)
    return g


@dataclass
class BNState:
    """What a BatchNorm node carries on the device (``nd.attrs["bn_state"]``).  Its statistics
    protocol (ops/hip.py: partials or accumulators) is decided once, by PlanExec._plan_bn_fin;
    the ops hand ``fwd`` and ``carry()`` to ops/hip.py without looking inside."""
    st: torch.Tensor  # [4][C] mean, invstd, scale, shift
    co: torch.Tensor  # [3][C] backward coefficients
    fwd: object  # what a forward consumer reads: st, or the BNFin that finalizes into it
    fwd_part: torch.Tensor  # fp32 [T][2][C] partials the forward turns into st with a bn_finalize launch, or None
    bwd: torch.Tensor  # the backward sums: fp32 [T][2][C] partials, or the int64 accumulator
    carrier: str = "part"  # the H.bn_bwd / H.pool_bn_bwd argument that takes bwd: "part" or "acc"
    dgrad: torch.Tensor = None  # bwd's like, written by the consuming conv's backprop-input (_plan_bn_dgrad_fusion)
    dgrad_fused: bool = False  # ... and this step's backprop-input did write it

    def carry(self, buf=None):
        """The part / acc arguments of H.bn_bwd / H.pool_bn_bwd for ``buf`` (default: bwd)."""
        return {"part": None, "acc": None, self.carrier: self.bwd if buf is None else buf}


class PlanExec:
    """The buffers of ``plan`` on ``device`` and the forward ops over them; weights come from
    ``params`` (a FlatParams over every variable the plan reads).
    ``bn_fin`` (with DAMD_BN_FIN, default on; per node, _plan_bn_fin): BatchNorm statistics through int64 fixed-point
    accumulators (order-independent: bitwise the same sums whatever order the producer blocks
    arrive in) finalized inside the consumer kernels (ops/hip.py BNFin): 40 fewer launches per
    ResNet-18 step.  Same-address fp64 atomics serialise at the memory side (~18 ns each: with
    one accumulator bn_bwd_reduce took 8.6 -> 26 us, the step 3.02 ms), so the producers add
    into DAMD_BN_REPS (8) replicas (block b -> replica b % 8) that the consumers sum in
    order: 2.665 vs 2.712 ms/step with the partials + finalize launches (DAMD_BN_FIN=0).
    ``weights_static``: the padded weight copies are made by the owner once per call
    (inference), not by every forward.  ``aug_training``: an input prefix flips and crops at
    random (False: flips off, crops centred)."""

    def __init__(self, plan, params, C, device, bn_fin: bool, weights_static: bool, aug_training: bool):
        self.plan, self.params, self.C, self.device = plan, params, C, device
        self.bn_fin, self.weights_static, self.aug_training = bn_fin, weights_static, aug_training
        self.B = plan.B
        self.ctrl = torch.zeros(32, dtype=torch.int32, device=device)  # the device Ctrl block
        self._allocate()
        # the first padded conv's bf16 weight copy (the packed-tap stem) is refreshed inside
        # the gather launch (no pad_cast launch of its own): nothing writes the masters
        # between this launch and that conv
        self.pad_folded = next((nd for nd in plan.live if self.pad_job(nd) is not None), None)
        # the logits layer's bias gradient comes out of the loss launch (no colsum launch;
        # DAMD_XENT_BIAS=0: the colsum launch, the same bits)
        last = plan.head_node
        last.attrs["bias_folded"] = (last.kind == "Dense" and last.layer.use_bias and "dz" not in last.attrs
                                     and H.softmax_bias_fold_ok(self.B, self.K)
                                     and env.get_bool("DAMD_XENT_BIAS", True))

    def _allocate(self):
        dev, plan = self.device, self.plan
        nbytes = 0

        def alloc(t: T, dtype=torch.bfloat16):
            nonlocal nbytes
            if t.alias_of is not None:
                return
            t.buf = torch.zeros(t.shape, dtype=dtype, device=dev)
            t.dtype = dtype
            nbytes += t.buf.numel() * t.buf.element_size()
            if t.needs_grad:
                t.grad = torch.zeros(t.shape, dtype=torch.bfloat16, device=dev)
                nbytes += t.grad.numel() * 2

        alloc(plan.x0)
        self.labels = torch.zeros(self.B, dtype=torch.int32, device=dev)
        last = plan.head_node
        if last is None:
            raise ValueError("native plan: " + plan.head_why)
        for nd in plan.nodes:
            if nd is last or nd.attrs.get("pool") is not None:  # stem-fused BN: no output tensor
                continue
            alloc(nd.out)
        # logits: fp32, row pitch padded to 8
        K = last.layer.units
        self.K, self.Kp = K, _pad8(K)
        self.logits = torch.zeros(self.B, self.Kp, dtype=torch.float32, device=dev)
        self.dlogits = torch.zeros(self.B, self.Kp, dtype=torch.bfloat16, device=dev)
        self.xent_rows = H.xent_rows(self.B, dev)  # fixed-order loss / metric sums
        # per-node scratch
        self._ident_cache = {}
        ws = 0  # fp32 split-K slabs, shared by every split GEMM (they run in order on one stream)
        for nd in plan.live:
            k = nd.kind
            if k == "Conv2D":
                l = nd.layer
                xshape = nd.inputs[0].root().shape
                kh, kw, cin0, cout = l.kernel.shape
                nd.attrs["cin_pad"] = cin = xshape[3]
                wshape = (kh, kw, cin, cout)
                wsh = wshape if cin != cin0 else None  # the padded weight copy's shape
                if cin == 4 and H.stem4_ok(xshape, wshape, l.strides, l.padding):
                    wsh = H.stem4_weight_shape(wshape)
                    nd.attrs["stem4"] = True
                if wsh is not None:
                    nd.attrs["w_pad"] = torch.zeros(wsh, dtype=torch.bfloat16, device=dev)
                    nd.attrs["dw_pad"] = torch.zeros(wsh, dtype=torch.float32, device=dev)
                fplan = H.conv_fwd_plan(xshape, wshape, l.strides, l.padding)
                ws = max(ws, H.conv_wgrad_workspace_elems(xshape, wshape, l.strides, l.padding), fplan["ws"],
                         H.conv_dgrad_plan(xshape, wshape, l.strides, l.padding)["ws"])
                if nd.attrs.get("stats"):
                    nd.attrs["stats_buf"] = torch.zeros(fplan["stats_T"], 2, cout, device=dev)
                if l.use_bias:  # bias gradient = column sums of dy, fixed order
                    ws = max(ws, H.colsum_workspace_elems(int(np.prod(nd.out.shape[:-1])), cout))
                if _act_name(l) != "linear":
                    nd.attrs["dz"] = torch.zeros(nd.out.shape, dtype=torch.bfloat16, device=dev)
            elif k == "DepthwiseConv2D":
                l = nd.layer
                nd.attrs["geo"] = g = H.pool_geo(nd.inputs[0].root().shape, l.kernel_size, l.strides, l.padding)
                ws = max(ws, H.dwconv_wgrad_workspace_elems(g))
                if l.use_bias:
                    ws = max(ws, H.colsum_workspace_elems(int(np.prod(nd.out.shape[:-1])), nd.out.shape[-1]))
                if _act_name(l) != "linear":
                    nd.attrs["dz"] = torch.zeros(nd.out.shape, dtype=torch.bfloat16, device=dev)
            elif k == "BatchNormalization":
                C = nd.out.shape[-1]
                M = int(np.prod(nd.out.shape[:-1]))
                st = torch.zeros(4, C, device=dev)
                part = torch.zeros(max(H.bn_bwd_blocks(M, C), 1), 2, C, device=dev)
                nd.attrs["bn_state"] = BNState(st, torch.zeros(3, C, device=dev), fwd=st, fwd_part=part, bwd=part)
                self._ident(C)  # (built here, not by the first step that needs it)
            elif k in ("Activation", "ReLU"):
                self._ident(nd.out.shape[-1])
            elif k == "MaxPooling2D":
                nd.attrs["arg"] = torch.zeros(nd.out.shape, dtype=torch.uint8, device=dev)
            elif k == "Dense":
                l = nd.layer
                kin, units = l.kernel.shape
                ws = max(ws, H.wgrad_workspace_elems(kin, _pad8(units), self.B),
                         H.dense_workspace_elems(self.B, _pad8(units), kin),
                         H.colsum_workspace_elems(self.B, units))
                if nd.attrs.get("logits") and units % 8:
                    up = _pad8(units)
                    nd.attrs["w_pad"] = torch.zeros(kin, up, dtype=torch.bfloat16, device=dev)
                    nd.attrs["dw_pad"] = torch.zeros(kin, up, dtype=torch.float32, device=dev)
                    if l.use_bias:
                        nd.attrs["b_pad"] = torch.zeros(up, dtype=torch.float32, device=dev)
                if _act_name(l) != "linear" and not nd.attrs.get("logits"):  # (a softmax head: in the loss)
                    nd.attrs["dz"] = torch.zeros(nd.out.shape, dtype=torch.bfloat16, device=dev)
        self._plan_bn_fin()
        self._plan_bn_dgrad_fusion()
        self._plan_bn_conv_fold()
        # one scratch bf16 buffer for "second writer" gradient accumulation
        big = max([int(np.prod(t.shape)) for t in self.plan.all_tensors()] + [1])
        self.scratch = torch.zeros(big, dtype=torch.bfloat16, device=dev)
        self.scratch2 = torch.zeros(big, dtype=torch.bfloat16, device=dev)
        nbytes += big * 4
        self.gemm_ws = torch.zeros(max(ws, 4), dtype=torch.float32, device=dev)
        nbytes += self.gemm_ws.numel() * 4
        self.act_bytes = nbytes

    def _plan_bn_fin(self):
        """The statistics protocol of every BatchNorm (the only place that decides it).  A node
        whose input's conv produces its statistics (stats_from_conv) gets accumulators: fixed
        point [2][C] forward sums the conv's epilogue adds into and [2][C] backward sums, all in
        one buffer cleared by the step's gather_batch launch.  Every other node keeps partials:
        it sums its input itself (H.bn_stats), and that kernel cannot write the forward
        accumulator layout."""
        bns = [nd for nd in self.plan.live if nd.kind == "BatchNormalization"]
        use = (self.bn_fin and env.get_bool("DAMD_BN_FIN", True)
               and all(nd.out.shape[-1] <= H.FIN_MAX_C for nd in bns))
        self.bn_acc = None
        bns = [nd for nd in bns if nd.attrs.get("stats_from_conv")]
        for nd in bns:  # (partials: the ones the conv's epilogue writes)
            nd.attrs["bn_state"].fwd_part = self.plan.producer(nd.inputs[0]).attrs["stats_buf"]
        if not use or not bns:
            return
        R = max(1, env.get_int("DAMD_BN_REPS", 8))
        # int64 fixed point (ops/hip.py bn_acc_encode): forward [R][2C] one word per value,
        # backward [R][4C] two words per value, each followed by its sticky flag plane
        # (damd_common.h bnacc_flag)
        tot = sum(6 * (R + 1) * nd.out.shape[-1] for nd in bns)
        self.bn_acc = torch.zeros(tot, dtype=torch.int64, device=self.device)
        o = 0
        for nd in bns:
            C, b, l = nd.out.shape[-1], nd.attrs["bn_state"], nd.layer
            nf, nb = 2 * C * (R + 1), 4 * C * (R + 1)
            acc_f = self.bn_acc[o:o + nf].view(R + 1, 2 * C)
            b.carrier, b.bwd = "acc", self.bn_acc[o + nf:o + nf + nb].view(R + 1, 4 * C)
            o += nf + nb
            self.plan.producer(nd.inputs[0]).attrs["stats_buf"] = acc_f
            M = int(np.prod(nd.inputs[0].shape[:-1]))
            b.fwd_part = None
            b.fwd = H.BNFin(acc_f, self.params.view(l.gamma), self.params.view(l.beta), b.st, l.moving_mean.value,
                            l.moving_variance.value, M, l.epsilon, l.momentum)

    def _bn_relu_convs(self):
        """(bn, conv) of every BN -> ReLU -> Conv2D chain with an own-pass BN + ReLU, the conv
        the ReLU output's only consumer and reading the unpadded weights."""
        for bn in self.plan.live:
            a = bn.attrs
            if bn.kind != "BatchNormalization" or not a.get("relu") or a.get("stats_only") or a.get("pool") is not None:
                continue
            outs = bn.out.consumers
            if len(outs) != 1 or not outs[0].attrs.get("dead") or len(outs[0].out.consumers) != 1:
                continue
            conv = outs[0].out.consumers[0]
            if conv.kind == "Conv2D" and not conv.attrs.get("dead") and "w_pad" not in conv.attrs:
                yield bn, conv

    def _plan_bn_dgrad_fusion(self):
        """BN -> ReLU -> Conv2D with the conv as the ReLU output's only consumer (the first
        conv of every ResNet basic block's second half): the conv's backprop-input, when the
        direct 3x3 kernel runs it, also writes the BN-backward partials in its epilogue
        (E_BNRED), so that BN's backward skips its reduce pass (one read of dy and x less)."""
        if not env.get_bool("DAMD_BN_DGRAD_FUSE", True) or not env.get_bool("DAMD_BN_MASK_FROM_X", True):
            return
        for bn, conv in self._bn_relu_convs():
            a, l = bn.attrs, conv.layer
            plan = H.conv_dgrad_plan(bn.out.shape, tuple(l.kernel.shape), l.strides, l.padding)
            if plan["amode"] != H.A_DGRAD3:
                continue
            # with the in-consumer finalize the epilogue adds into the fixed-point accumulator
            b = a["bn_state"]
            b.dgrad = (b.bwd if b.carrier == "acc" else
                       torch.zeros(plan["stats_T"], 2, bn.out.shape[-1], device=self.device))
            conv.attrs["bnred"] = bn

    def _plan_bn_conv_fold(self):
        """BN -> ReLU -> Conv2D with the conv as the ReLU output's only consumer and a direct
        3x3 forward plan (the second conv of every ResNet basic block on layers 1-3): the conv
        reads the BN INPUT, finalizes the statistics and applies BN + ReLU to its staged halo
        in LDS, and stores y for the weight gradient -- the bn_apply launch (a read of x and a
        write of y) disappears.  Needs the in-consumer finalize (bn_acc).  DAMD_BN_CONV_FOLD=0
        keeps the apply launch."""
        if self.bn_acc is None or not env.get_bool("DAMD_BN_CONV_FOLD", True):
            return
        for bn, conv in self._bn_relu_convs():
            a, l = bn.attrs, conv.layer
            if a["bn_state"].carrier != "acc" or conv.attrs.get("stem4") or conv.inputs[0].root() is not bn.out.root():
                continue
            plan = H.conv_fwd_plan(tuple(bn.out.shape), tuple(l.kernel.shape), l.strides, l.padding)
            if plan["amode"] != H.A_CONV3 or plan["splits"] != 1:
                continue
            a["conv_fold"] = conv
            conv.attrs["bnin"] = bn

    def _ident(self, C):
        """[4, C] rows (mean 0, invstd 1, scale 1, shift 0): bn_apply as a plain ReLU, and
        bn_bwd_reduce as a sum / sum of squares."""
        t = self._ident_cache.get(C)
        if t is None:
            t = self._ident_cache[C] = torch.zeros(4, C, device=self.device)
            t[1:3].fill_(1.0)
        return t

    # --- forward ops ------------------------------------------------------------------------
    def forward(self):
        for nd in self.plan.live:
            getattr(self, "_fwd_" + nd.kind)(nd)

    def _fwd_Conv2D(self, nd):
        l = nd.layer
        x = nd.inputs[0].root().buf
        wb = self.params.bview(l.kernel)
        bias = self.params.view(l.bias) if l.use_bias else None
        relu = getattr(l.activation, "__name__", "linear") == "relu"
        if not self.weights_static and nd is not self.pad_folded:
            self.pad_weights(nd)
        if nd.attrs.get("stem4"):
            kh = l.kernel.shape[0]
            wp = nd.attrs["w_pad"]
            H.conv_fwd_stem4(x, wp, nd.out.root().buf, kh, l.strides, l.padding, bias=bias, relu=relu,
                             stats=nd.attrs.get("stats_buf"), workspace=self.gemm_ws)
        else:
            if "w_pad" in nd.attrs:
                wb = nd.attrs["w_pad"]
            bn = nd.attrs.get("bnin")  # BN -> ReLU of the input applied on load (_plan_bn_conv_fold)
            H.conv_fwd(bn.inputs[0].root().buf if bn is not None else x, wb, nd.out.root().buf, l.strides, l.padding,
                       bias=bias, relu=relu, stats=nd.attrs.get("stats_buf"), workspace=self.gemm_ws,
                       bnin=(bn.attrs["bn_state"].fwd, x) if bn is not None else None)
        self._act_epilogue(nd)

    def _fwd_DepthwiseConv2D(self, nd):
        # (also the depthwise half of a SeparableConv2D: no bias, linear)
        l = nd.layer
        bias = self.params.view(l.bias) if l.use_bias else None
        H.dwconv_fwd(nd.inputs[0].root().buf, self.params.bview(l.depthwise_kernel), bias,
                     _act_name(l) == "relu", nd.attrs["geo"], nd.out.root().buf)
        self._act_epilogue(nd)

    def pad_job(self, nd):
        """(fp32 master view, padded bf16 copy, R, C1, C2, C1p, C2p) of a padded conv's
        pad_cast, or None."""
        if nd.kind != "Conv2D" or "w_pad" not in nd.attrs:
            return None
        kh, kw, cin, cout = nd.layer.kernel.shape
        src, dst = self.params.view(nd.layer.kernel), nd.attrs["w_pad"]
        if nd.attrs.get("stem4"):
            # [KH][KW][cin][cout] -> [KH][8][4][cout]: the (cin, cout) rows padded at their tail
            return (src, dst, kh, kw, cin * cout, 8, 4 * cout)
        return (src, dst, kh * kw, cin, cout, nd.attrs["cin_pad"], cout)

    def pad_weights(self, nd):
        """Refresh a layer's padded bf16 weight copy from the fp32 masters (every training
        step; once per call for an inference plan, whose weights do not move)."""
        l = nd.layer
        if "w_pad" not in nd.attrs:
            return
        if nd.kind == "Conv2D":
            src, dst, *dims = self.pad_job(nd)
            H.pad_cast(src, *dims, dst)
        elif nd.kind == "Dense":
            kin, units = l.kernel.shape
            H.pad_cast(self.params.view(l.kernel), 1, kin, units, kin, nd.attrs["w_pad"].shape[1], nd.attrs["w_pad"])
            if l.use_bias:
                nd.attrs["b_pad"][:units].copy_(self.params.view(l.bias))

    def _act_epilogue(self, nd):
        """sigmoid / tanh of a Conv2D / Dense: in place over the GEMM's bf16 output (ReLU
        rides in the GEMM epilogue itself)."""
        an = _act_name(nd.layer)
        if an in ("sigmoid", "tanh"):
            y = nd.out.root().buf
            H.act_fwd(y, y, an)

    def _fwd_BatchNormalization(self, nd):
        l, b = nd.layer, nd.attrs["bn_state"]
        x = nd.inputs[0].root()
        # inference: the moving statistics; the owner fills st (H.bn_infer_st) once per call
        if not self.plan.inference and b.fwd_part is not None:
            Tn = b.fwd_part.shape[0]
            if not nd.attrs.get("stats_from_conv"):  # sum / sum of squares of x
                Tn = H.bn_stats(x.buf, self._ident(x.shape[-1]), b.fwd_part)
            H.bn_finalize(b.fwd_part, Tn, x.shape[-1], int(np.prod(x.shape[:-1])), self.params.view(l.gamma),
                          self.params.view(l.beta), l.epsilon, l.momentum, l.moving_mean.value,
                          l.moving_variance.value, b.st)
        if nd.attrs.get("stats_only") or nd.attrs.get("pool") is not None or nd.attrs.get("conv_fold"):
            return  # (finalized and) applied by the fused Add / MaxPool / direct conv that consumes it
        H.bn_apply(x.buf, b.fwd, nd.out.root().buf, relu=nd.attrs.get("relu", False))

    def _fwd_Activation(self, nd):
        C = nd.out.shape[-1]
        x = nd.inputs[0].root()
        an = _act_name(nd.layer) if nd.kind == "Activation" else "relu"
        if an == "relu" and C % 8 == 0:
            H.bn_apply(x.buf, self._ident(C), nd.out.root().buf, relu=True)
        else:
            H.act_fwd(x.buf, nd.out.root().buf, an)

    def _fwd_Augment(self, nd):
        H.augment(self.plan.x0.buf, nd.out.buf, self.labels, self.ctrl, nd.attrs["table"], self.aug_training)

    def _fwd_Dropout(self, nd):
        H.dropout(nd.inputs[0].root().buf, nd.out.root().buf, self.ctrl, nd.attrs["seed"], nd.layer.rate)

    def _fwd_AveragePooling2D(self, nd):
        l = nd.layer
        H.avgpool_fwd(nd.inputs[0].root().buf, nd.out.root().buf, l.pool_size, l.strides, l.padding)

    _fwd_ReLU = _fwd_Activation

    def _fwd_Add(self, nd):
        fused = nd.attrs.get("fused")
        if fused is None:
            a, b = nd.inputs[0].root().buf, nd.inputs[1].root().buf
            H.add_bf16(a, b, nd.out.root().buf)
            return
        main, (mode, other) = fused
        x = main.inputs[0].root()
        if mode == "raw":
            r, st2 = other.root().buf, None
        else:
            r, st2 = other.inputs[0].root().buf, other.attrs["bn_state"].fwd
        H.bn_apply(x.buf, main.attrs["bn_state"].fwd, nd.out.root().buf, relu=nd.attrs.get("relu", False), r=r,
                   st2=st2)

    def _fwd_MaxPooling2D(self, nd):
        l = nd.layer
        bn = nd.attrs.get("bn")
        if bn is not None:  # stem fusion: pool(relu(BN(x))) straight from the conv output
            H.bn_relu_maxpool_fwd(bn.inputs[0].root().buf, bn.attrs["bn_state"].fwd, nd.out.root().buf,
                                  nd.attrs["arg"], l.pool_size, l.strides, l.padding)
            return
        H.maxpool_fwd(nd.inputs[0].root().buf, nd.out.root().buf, nd.attrs["arg"], l.pool_size, l.strides, l.padding)

    def _fwd_GlobalAveragePooling2D(self, nd):
        H.gap_fwd(nd.inputs[0].root().buf, nd.out.root().buf)

    def _fwd_Dense(self, nd):
        l = nd.layer
        x = nd.inputs[0].root().buf
        x2 = x.view(x.shape[0], -1)
        wb = self.params.bview(l.kernel)
        bias = self.params.view(l.bias) if l.use_bias else None
        if not self.weights_static:
            self.pad_weights(nd)
        if "w_pad" in nd.attrs:
            wb = nd.attrs["w_pad"]
            if bias is not None:
                bias = nd.attrs["b_pad"]
        relu = getattr(l.activation, "__name__", "linear") == "relu"
        out = self.logits if nd.attrs.get("logits") else nd.out.root().buf
        H.dense_fwd(x2, wb, out, bias=bias, relu=relu, workspace=self.gemm_ws)
        if not nd.attrs.get("logits"):
            self._act_epilogue(nd)
