"""The device-free half of the native engines (planner inspection and CPU tests need no GPU):
the eligibility rules, the layer graph and its output head, :func:`lower` -- a Keras model as
a :class:`Plan` of fused nodes over planned tensors -- and :func:`plan_buckets`.

Fusion rules (decided on the layer graph, not traced):
  Conv2D(no bias, linear) -> BatchNormalization : batch statistics from the conv epilogue
  BatchNormalization -> ReLU                    : ReLU in the BN apply
  BatchNormalization -> Add(other) [-> ReLU]    : residual add (+ the other branch's own
                                                  BN when it is BN-terminated) in one pass

With DAMD_NATIVE_DEPTHWISE=1 (off by default) DepthwiseConv2D plans as a node of its own and
SeparableConv2D as two: a DepthwiseConv2D node (no bias, linear) and a 1 x 1 Conv2D node over
a planned intermediate tensor, so the rules above apply to the pointwise half unchanged.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from ..ops import hip as H
from ..utils import env


def _pad8(c):
    return -(-c // 8) * 8


@dataclass
class T:
    """A planned tensor (per-replica batch)."""

    shape: tuple
    dtype: torch.dtype = torch.bfloat16
    buf: Optional[torch.Tensor] = None
    grad: Optional[torch.Tensor] = None
    needs_grad: bool = True
    alias_of: Optional["T"] = None
    consumers: List["Node"] = field(default_factory=list)
    written: bool = False  # backward bookkeeping

    def root(self):
        t = self
        while t.alias_of is not None:
            t = t.alias_of
        return t


@dataclass
class Node:
    kind: str
    layer: object
    inputs: List[T]
    out: T
    attrs: Dict = field(default_factory=dict)


def _layer_graph(model):
    """[(layer, [input keys], output key)], input key, output key."""
    from ..keras import layers as L

    if hasattr(model, "_layers") and not getattr(model, "_nodes", None):
        ls = [l for l in model._layers if not isinstance(l, L.InputLayer)]
        seq = []
        for i, l in enumerate(ls):
            seq.append((l, [i], i + 1))
        return seq, 0, len(ls), tuple(model.input_shape[1:])
    keys = {id(model._inputs[0]): 0}
    seq = []
    for t in model._nodes:
        keys[id(t)] = len(keys)
        seq.append((t.layer, [keys[id(i)] for i in t.inputs], keys[id(t)]))
    return seq, 0, keys[id(model._outputs[0])], tuple(model._inputs[0].shape[1:])


def input_prefix(seq, in_key):
    """The model's input prefix: the maximal chain of ZeroPadding2D / RandomCrop / RandomFlip
    entries of ``seq`` that starts at the model input, each reading a tensor nobody else
    reads -- what the ``augment`` kernel runs as one launch behind ``gather_batch``."""
    chain, key = [], in_key
    while True:
        users = [e for e in seq if key in e[1]]
        if len(users) != 1 or type(users[0][0]).__name__ not in H.AUG_LAYERS or len(users[0][1]) != 1:
            return chain
        chain.append(users[0])
        key = users[0][2]


def _act_name(layer) -> str:
    act = getattr(layer, "activation", None)
    return getattr(act, "__name__", "linear") if act is not None else "linear"


def _is_softmax(layer) -> bool:
    k = type(layer).__name__
    return k == "Softmax" or (k == "Activation" and _act_name(layer) == "softmax")


def output_head(seq):
    """The output head of a layer graph (``_layer_graph``'s ``seq``): (kind, Dense layer,
    terminal softmax layer or None, reason).  kind is

    * ``'logits'``: the model ends in a linear Dense;
    * ``'probs'``: the last Dense has ``activation='softmax'``, or a linear Dense is followed
      by a terminal ``Softmax()`` / ``Activation('softmax')``;
    * None (with the reason) for anything else.

    Either way the native plan produces the fp32 logits of that Dense: a terminal softmax
    lives in the loss kernel (training, evaluate) or the ``softmax_store`` tail (predict)."""
    last, ins, _ = seq[-1]
    if _is_softmax(last):
        prod = [e[0] for e in seq if e[2] == ins[0]] if len(ins) == 1 else []
        users = [e for e in seq if ins[0] in e[1]] if len(ins) == 1 else []
        if (len(prod) == 1 and len(users) == 1 and type(prod[0]).__name__ == "Dense"
                and _act_name(prod[0]) == "linear"):
            return "probs", prod[0], last, ""
        return None, None, None, "a terminal softmax must follow a linear Dense"
    if type(last).__name__ == "Dense" and _act_name(last) == "linear":
        return "logits", last, None, ""
    if type(last).__name__ == "Dense" and _act_name(last) == "softmax":
        return "probs", last, None, ""
    return None, None, None, "the model must end in a linear Dense (logits) or a softmax over one"


def loss_head_ok(model, head_kind):
    """(ok, reason): the compiled loss and metrics are ones the device loss head computes for
    a model whose output is ``head_kind`` ('logits' / 'probs').

    Sparse and categorical cross-entropy (label smoothing in [0, 1)) with ``from_logits``
    matching the head; metrics by class: SparseCategoricalAccuracy with the sparse loss,
    CategoricalAccuracy with the categorical one (what 'accuracy' / 'acc' resolve to).

    For a 'probs' head the loss and its gradient are computed from the logits, as tf.keras
    does for softmax-terminated models.  That equals the PyTorch path's ``per_sample`` on
    the probabilities except where a probability leaves [1e-7, 1 - 1e-7], which that path
    clips and this one does not."""
    from ..keras import losses, metrics

    loss = model.loss
    if isinstance(loss, losses.SparseCategoricalCrossentropy):
        want = metrics.SparseCategoricalAccuracy
    elif isinstance(loss, losses.CategoricalCrossentropy):
        want = metrics.CategoricalAccuracy
        eps = float(loss.label_smoothing or 0.0)
        if not 0.0 <= eps < 1.0:
            return False, f"label_smoothing {eps} outside [0, 1)"
    else:
        return False, "loss"
    if head_kind == "probs" and loss.from_logits:
        return False, "from_logits=True on a softmax output would apply softmax twice"
    if head_kind == "logits" and not loss.from_logits:
        return False, "from_logits=False on a linear (logits) output"
    for m in model.compiled_metrics:
        if not isinstance(m, want):
            return False, f"metric {m.name} ({type(m).__name__}) with {type(loss).__name__}"
    return True, ""


def dense_targets(model) -> bool:
    """The compiled loss takes dense [n, K] target rows (one-hot / soft), not class ids."""
    from ..keras import losses

    return isinstance(model.loss, losses.CategoricalCrossentropy)


def _param_weights(model):
    """Every layer weight the forward plan reads (kernels, biases, BN gamma / beta),
    trainable or frozen -- i.e. all weights except the BN moving statistics."""
    out = []
    for l in model.layers:
        stats = {id(getattr(l, "moving_mean", None)), id(getattr(l, "moving_variance", None))}
        out += [w for w in l.weights if id(w) not in stats]
    return out


def reg_rows(variables, offsets):
    """Segment-table rows (offset, size, l1, l2) of the L1L2-regularized ``variables`` laid
    out at ``offsets`` of a flat buffer (an L1L2 with both coefficients 0 has no row)."""
    from ..keras import regularizers as _regs

    rows = []
    for v, off in zip(variables, offsets):
        co = _regs.coefficients(getattr(v, "regularizer", None))
        if co is not None and (co[0] or co[1]):
            rows.append((off, int(np.prod(v.shape)), co[0], co[1]))
    return rows


def regularizers_ok(model):
    """(ok, reason): every weight penalty of ``model`` is an L1L2 (the closed form the
    opt_step / reg_penalty kernels implement) and they fit the segment table."""
    from ..keras import regularizers as _regs

    regs = model._regularized()
    for v, r in regs:
        if _regs.coefficients(r) is None:
            return False, f"regularizer {_regs.name_of(r)}"
    if len(regs) > H.REG_MAX_ROWS:
        return False, f"regularizers: {len(regs)} segments exceed the table cap {H.REG_MAX_ROWS}"
    return True, ""


def clipping_ok(model):
    """(ok, reason): the optimizer's gradient clipping has a native form.  clipvalue and
    global_clipnorm always do; clipnorm looks up each element's variable in opt_step's
    LDS-staged table, which then lists every trainable variable."""
    mode, c = model.optimizer.clipping()
    if mode is None:
        return True, ""
    if not (np.isfinite(c) and c > 0.0):
        return False, f"{mode} {c!r} is not a finite number > 0"
    nvar = len(model.trainable_weights)
    if mode == "clipnorm" and nvar > H.REG_MAX_ROWS:
        return False, f"clipnorm: {nvar} variables exceed the table cap {H.REG_MAX_ROWS}"
    return True, ""


def _schedule_of(opt):
    """The optimizer's learning-rate schedule, or None for a plain number."""
    from ..keras.schedules import LearningRateSchedule

    lr = opt.learning_rate
    return lr if isinstance(lr, LearningRateSchedule) else None


def schedule_ok(model):
    """(ok, reason): the optimizer's learning rate has a native form.  A number always does
    (ctrl's lr); a schedule when opt_step's descriptor holds it (ops/hip.py lr_schedule_ok):
    one of the five keras/schedules.py classes with integral step counts in range, at most
    H.LR_MAX_BOUNDS integer boundaries and finite parameters."""
    sched = _schedule_of(model.optimizer)
    if sched is None:
        return True, ""
    return H.lr_schedule_ok(sched)


def _opt_kernel_slots(opt):
    """(opt_step kind, slot names for S0..S2; '' = unused) of a Keras optimizer."""
    from ..keras import optimizers

    if isinstance(opt, optimizers.Adam):
        return 1, ["m", "v", "vhat" if opt.amsgrad else ""]
    if isinstance(opt, optimizers.RMSprop):
        return 2, ["rms", "momentum" if opt.momentum else "", "mg" if opt.centered else ""]
    return 0, ["momentum" if opt.momentum else "", "", ""]


SUPPORTED = ("Conv2D", "BatchNormalization", "Activation", "ReLU", "Add", "MaxPooling2D",
             "AveragePooling2D", "GlobalAveragePooling2D", "Flatten", "Dense", "Dropout")
ACTIVATIONS = ("linear", "relu", "sigmoid", "tanh")
# with DAMD_NATIVE_DEPTHWISE=1 (off by default): csrc/kernels/dwconv.hip, depth_multiplier 1
DEPTHWISE = ("DepthwiseConv2D", "SeparableConv2D")


def native_depthwise() -> bool:
    return env.get_bool("DAMD_NATIVE_DEPTHWISE", False)


def _depthwise_ok(k, l):
    """(ok, reason) of a DepthwiseConv2D / SeparableConv2D layer for the dwconv kernels."""
    if l.depth_multiplier != 1:
        return False, f"depthwise depth_multiplier {l.depth_multiplier}"
    ks, st = tuple(l.kernel_size), tuple(l.strides)
    if (tuple(l.dilation_rate) != (1, 1) or ks[0] != ks[1] or ks[0] > H.DWCONV_MAX_K or st[0] != st[1]
            or st[0] not in (1, 2)):
        return False, "depthwise geometry"
    if l.depthwise_kernel.shape[2] % 8:
        return False, "depthwise input channels must be a multiple of 8"
    if k == "SeparableConv2D" and l.filters % 8:
        return False, "separable filters must be a multiple of 8"
    an = _act_name(l)
    if an not in ACTIVATIONS:
        return False, f"activation {an}"
    return True, ""


class SeparableDepthwise:
    """The depthwise half of a SeparableConv2D as a DepthwiseConv2D node's layer (read-only):
    the layer's kernel size, strides and padding; no bias, linear."""
    use_bias, bias, activation, depth_multiplier, dilation_rate = False, None, None, 1, (1, 1)

    def __init__(self, layer):
        self.layer, self.name = layer, layer.name + "/depthwise"

    depthwise_kernel = property(lambda self: self.layer.depthwise_kernel)
    kernel_size = property(lambda self: tuple(self.layer.kernel_size))
    strides = property(lambda self: tuple(self.layer.strides))
    padding = property(lambda self: self.layer.padding)


class SeparablePointwise:
    """The pointwise half of a SeparableConv2D as a Conv2D node's layer (read-only): a 1 x 1
    'valid' convolution by ``pointwise_kernel`` with the layer's bias and activation."""
    kernel_size, strides, padding, dilation_rate = (1, 1), (1, 1), "valid", (1, 1)

    def __init__(self, layer):
        self.layer, self.name = layer, layer.name + "/pointwise"

    kernel = property(lambda self: self.layer.pointwise_kernel)
    filters = property(lambda self: self.layer.filters)
    use_bias = property(lambda self: self.layer.use_bias)
    bias = property(lambda self: self.layer.bias)
    activation = property(lambda self: self.layer.activation)


def layers_eligible(model):
    """(ok, reason): every layer of ``model`` has a native forward + backward kernel
    and the model ends in one of the heads of :func:`output_head` (a linear Dense, a
    softmax Dense, or a linear Dense under a terminal softmax layer).  A softmax
    anywhere else has no kernel."""
    try:
        seq, in_key, out_key, in_shape = _layer_graph(model)
    except Exception as e:  # pragma: no cover
        return False, f"graph: {e}"
    if len(in_shape) != 3:
        return False, "input must be an image (H, W, C)"
    head_kind, head_dense, head_softmax, head_why = output_head(seq)
    prefix = input_prefix(seq, in_key)
    if len(prefix) > H.AUG_MAX_STAGES:
        return False, (f"input prefix: {len(prefix)} augmentation stages exceed the cap AUG_MAX_STAGES = "
                       f"{H.AUG_MAX_STAGES}")
    in_prefix = {id(e[0]) for e in prefix}
    for l, ins, _ in seq:
        k = type(l).__name__
        if l is head_softmax:
            continue  # planned away: the loss / predict tail applies it
        if id(l) in in_prefix:
            continue  # one augment launch behind gather_batch
        if k in H.AUG_LAYERS:
            return False, f"layer {k} is native only ahead of the first weight layer"
        if k not in SUPPORTED and not (k in DEPTHWISE and native_depthwise()):
            return False, f"layer {k}"
        if k in DEPTHWISE:
            ok, why = _depthwise_ok(k, l)
            if not ok:
                return False, why
        an = _act_name(l)
        if (k in ("Conv2D", "Dense", "Activation") and an not in ACTIVATIONS
                and l is not head_dense):
            return False, f"activation {an}"
        if k == "ReLU" and (l.max_value is not None or l.negative_slope or l.threshold):
            return False, "ReLU options"
        if k == "Conv2D":
            if l.dilation_rate != (1, 1) or l.kernel_size[0] != l.kernel_size[1] or l.strides[0] != l.strides[1]:
                return False, "conv geometry"
            if l.strides[0] not in (1, 2) or l.filters % 8:
                return False, "conv stride/filters"
        if k == "MaxPooling2D" and l.pool_size[0] * l.pool_size[1] > 255:
            return False, "pool size"
        if k == "Dropout" and not 0.0 <= l.rate < 1.0:
            return False, "dropout rate"
        if k == "BatchNormalization" and l.axis not in (-1, 3):
            return False, "BN axis"
        if k == "Add" and len(ins) != 2:
            return False, "Add arity"
        if k == "Dense" and l is not seq[-1][0] and l is not head_dense and l.units % 8:
            return False, "hidden Dense units must be a multiple of 8"
    if head_kind is None:
        return False, head_why
    return True, ""


class Plan:
    """A model lowered at one per-replica batch (made by :func:`lower`): ``nodes``, one per
    layer in execution order (``live``: those not fused away), over planned tensors from ``x0``
    (the gathered batch, ``cin_pad`` channels) to ``logits_t``, the output of ``head_node``."""

    def __init__(self, model, batch: int, rank: int, inference: bool):
        self.model, self.B, self.rank, self.inference = model, batch, rank, inference

    def _build(self):
        model, B = self.model, self.B
        seq, in_key, out_key, in_shape = _layer_graph(model)
        tensors: Dict[int, T] = {}
        h, w, c = in_shape
        self.in_shape = (h, w, c)
        self.cin_pad = _pad8(c)
        x0 = T((B, h, w, self.cin_pad), needs_grad=False)
        tensors[in_key] = x0
        self.x0 = x0
        nodes = []
        # the input prefix (ZeroPadding2D / RandomCrop / RandomFlip chain at the input): ONE
        # node whatever its length, x0 -> the augmented batch, no gradient, no backward work
        prefix = input_prefix(seq, in_key)
        aug = None
        if prefix:
            from ..keras.layers import augment_seeds

            stages, ho, wo = H.aug_stages([e[0] for e in prefix], augment_seeds(model), h, w)
            aug = Node("Augment", prefix[0][0], [x0], T((B, ho, wo, self.cin_pad), needs_grad=False),
                       {"layers": [e[0] for e in prefix], "stages": stages, "table": H.aug_table(stages)})
            x0.consumers.append(aug)
            tensors[prefix[-1][2]] = aug.out
            nodes.append(aug)
        for layer, ins, ok in seq:
            if any(layer is e[0] for e in prefix):
                continue
            kind = type(layer).__name__
            xs = [tensors[i] for i in ins]
            if kind == "SeparableConv2D":
                # two nodes over a planned bf16 intermediate: the depthwise half (no bias,
                # linear), then a 1 x 1 Conv2D by the pointwise kernel with the layer's bias and
                # activation -- every Conv2D rule (BN-statistics epilogue, ...) applies to it
                dw = SeparableDepthwise(layer)
                mid = Node("DepthwiseConv2D", dw, xs, T(self._out_shape("DepthwiseConv2D", dw, xs)))
                for x in xs:
                    x.consumers.append(mid)
                nodes.append(mid)
                kind, layer, xs = "Conv2D", SeparablePointwise(layer), [mid.out]
            shp = self._out_shape(kind, layer, xs)
            out = T(shp)
            nd = Node(kind, layer, xs, out)
            for x in xs:
                x.consumers.append(nd)
            tensors[ok] = out
            nodes.append(nd)
        self.logits_t = tensors[out_key]
        self.nodes = nodes
        self._producers = {id(nd.out): nd for nd in nodes}
        # the output head: the Dense whose fp32 logits feed the loss; a terminal softmax
        # layer is planned away (dead, aliasing the logits)
        self.head_kind, head_dense, head_softmax, self.head_why = output_head(seq)
        self.head_node = next((nd for nd in nodes if nd.layer is head_dense), None)
        if self.head_node is not None:
            self.head_node.attrs["logits"] = True
        if head_softmax is not None:
            sm = next(nd for nd in nodes if nd.layer is head_softmax)
            sm.attrs["dead"] = True
            sm.out.alias_of = sm.inputs[0]
        # packed-tap stem: a <= 4-channel input read only by stride-2 convs of <= 8 columns
        # is stored with 4 channels and those convs run K = KH x 32 (ops/hip.py stem4_ok)
        # (behind an input prefix the decision is the augmented tensor's consumers' and is
        # carried back to x0: the augment kernel moves whole pixels of either pitch)
        xin = aug.out if aug is not None else x0
        if c <= 4 and xin.consumers and env.get_bool("DAMD_STEM4", True) and all(
                nd.kind == "Conv2D" and H.stem4_ok(xin.shape[:3] + (4,),
                                                    (nd.layer.kernel.shape[0], nd.layer.kernel.shape[1],
                                                     4, nd.layer.kernel.shape[3]),
                                                    nd.layer.strides, nd.layer.padding)
                for nd in xin.consumers):
            self.cin_pad = 4
            x0.shape = (B, h, w, 4)
            xin.shape = xin.shape[:3] + (4,)
        self._fuse()

    def _out_shape(self, kind, l, xs):
        x = xs[0].shape
        B = self.B
        if kind == "Conv2D":
            ho, _ = H.conv_out(x[1], l.kernel_size[0], l.strides[0], l.padding)
            wo, _ = H.conv_out(x[2], l.kernel_size[1], l.strides[1], l.padding)
            return (B, ho, wo, l.filters)
        if kind == "DepthwiseConv2D":
            ho, _ = H.conv_out(x[1], l.kernel_size[0], l.strides[0], l.padding)
            wo, _ = H.conv_out(x[2], l.kernel_size[1], l.strides[1], l.padding)
            return (B, ho, wo, x[3])
        if kind in ("MaxPooling2D", "AveragePooling2D"):
            g = H.pool_geo(x, l.pool_size, l.strides, l.padding)
            return (B, g[10], g[11], x[3])
        if kind == "GlobalAveragePooling2D":
            return (B, x[3])
        if kind == "Flatten":
            return (B, int(np.prod(x[1:])))
        if kind == "Dense":
            return (B, l.units)
        return x

    def _fuse(self):
        def relu_node(nd):
            if nd.kind == "ReLU":
                return True
            return nd.kind == "Activation" and getattr(nd.layer.activation, "__name__", "") == "relu"

        for i, nd in enumerate(self.nodes):
            nd.attrs.setdefault("dead", False)
            if nd.kind == "Activation" and _act_name(nd.layer) == "linear":
                nd.attrs["dead"] = True  # linear activation: identity
                nd.out.alias_of = nd.inputs[0]
            if nd.kind == "Dropout":
                if nd.layer.rate == 0.0:
                    nd.attrs["dead"] = True
                    nd.out.alias_of = nd.inputs[0]
                # per-layer, per-replica mask stream (TF draws independent masks per replica)
                s0 = nd.layer.seed if getattr(nd.layer, "seed", None) is not None else 0x5EED
                nd.attrs["seed"] = (int(s0) * 0x9E3779B1 + (i + 1) * 0x85EBCA77
                                    + self.rank * 0xC2B2AE3D) & 0xFFFFFFFF
            if nd.kind == "Flatten":
                nd.attrs["dead"] = True  # NHWC flatten is a view
                nd.out.alias_of = nd.inputs[0]
        for nd in self.nodes:
            if nd.kind != "BatchNormalization":
                continue
            x = nd.inputs[0]
            prod = self.producer(x)
            if (prod is not None and prod.kind == "Conv2D" and not prod.layer.use_bias
                    and getattr(prod.layer.activation, "__name__", "linear") == "linear" and len(x.consumers) == 1):
                prod.attrs["stats"] = True
                nd.attrs["stats_from_conv"] = True
        for nd in self.nodes:
            if nd.kind != "BatchNormalization" or nd.attrs.get("stats_only"):
                continue
            y = nd.out
            if len(y.consumers) == 1 and y.consumers[0].kind == "Add":
                # BN -> Add(other) [-> ReLU]: one pass at the Add's position (after both branches)
                add = y.consumers[0]
                other = add.inputs[1] if add.inputs[0] is y else add.inputs[0]
                op = self.producer(other)
                nd.attrs["stats_only"] = True
                if (op is not None and op.kind == "BatchNormalization" and len(other.consumers) == 1
                        and not op.attrs.get("stats_only")):
                    op.attrs["stats_only"] = True
                    add.attrs["fused"] = (nd, ("bn", op))
                else:
                    add.attrs["fused"] = (nd, ("raw", other))
                out = add.out
                if len(out.consumers) == 1 and relu_node(out.consumers[0]):
                    r = out.consumers[0]
                    add.attrs["relu"] = True
                    r.attrs["dead"] = True
                    r.out.alias_of = out
                continue
            if len(y.consumers) == 1 and relu_node(y.consumers[0]):
                r = y.consumers[0]
                nd.attrs["relu"] = True
                r.attrs["dead"] = True
                r.out.alias_of = y
                # BN -> ReLU -> MaxPool (the ResNet stem): the pool normalises on the fly and
                # the BN+ReLU output is never stored (pool.hip stem fusion); its backward reduce
                # holds one 8-channel group per thread, so wider layers keep the unfused pair
                outs = r.out.consumers
                if (len(outs) == 1 and outs[0].kind == "MaxPooling2D" and y.shape[-1] <= H.STEM_FUSE_MAX_C
                        and env.get_bool("DAMD_STEM_FUSE", True)):
                    nd.attrs["pool"] = outs[0]
                    outs[0].attrs["bn"] = nd

    def _strip_training(self):
        """What a forward-only plan drops: Dropout is the identity, BatchNorm reads its
        moving statistics (no batch statistics from the convs), nothing needs a gradient."""
        for nd in self.nodes:
            if nd.kind == "Dropout" and not nd.attrs.get("dead"):
                nd.attrs["dead"] = True  # identity at inference
                nd.out.alias_of = nd.inputs[0]
            nd.attrs.pop("stats", None)  # BN uses the moving statistics: no batch statistics
            nd.attrs.pop("stats_from_conv", None)
        for t in self.all_tensors():
            t.needs_grad = False

    def producer(self, t):
        """The node whose output is tensor ``t`` (None for x0)."""
        return self._producers.get(id(t))

    def all_tensors(self):
        return [self.x0] + [nd.out for nd in self.nodes]

    def describe(self) -> dict:
        return {
            "nodes": len(self.nodes),
            "kernels_fwd": len(self.live),
            "conv_bn_stats": sum(1 for nd in self.nodes if nd.attrs.get("stats")),
            "bn_relu": sum(1 for nd in self.nodes if nd.kind == "BatchNormalization" and nd.attrs.get("relu")),
            "add_fused_raw": sum(1 for nd in self.nodes if nd.attrs.get("fused") and nd.attrs["fused"][1][0] == "raw"),
            "add_fused_bn": sum(1 for nd in self.nodes if nd.attrs.get("fused") and nd.attrs["fused"][1][0] == "bn"),
            "add_relu": sum(1 for nd in self.nodes if nd.kind == "Add" and nd.attrs.get("relu")),
            "dead": sum(1 for nd in self.nodes if nd.attrs.get("dead")),
            # rows of the weight-regularizer segment table (one per L1L2-regularized variable)
            "reg_segments": len(reg_rows(self.model.trainable_weights, range(len(self.model.trainable_weights)))),
        }

    describe_plan = describe  # (the name on the engine; what plan_only's callers use)


def lower(model, batch: int, *, rank: int = 0, inference: bool = False) -> Plan:
    """The fused plan of ``model`` at per-replica batch ``batch``.  ``rank`` enters the Dropout
    seeds only; ``inference``: the forward-only plan of predict / evaluate."""
    plan = Plan(model, batch, rank, inference)
    plan._build()
    if inference:
        plan._strip_training()
    plan.live = [nd for nd in plan.nodes if not nd.attrs.get("dead")]
    return plan


# --- gradient buckets (all-reduce overlapped with the rest of backward) ----------------------
def plan_buckets(plan, variables, sizes, offsets, total_elems: int, bucket_mb: float, last_mb: float = 1.0):
    """(buckets, writes) over the flat gradient buffer G of ``total_elems`` words: ``variables``
    (``sizes`` elements each, at ``offsets``), then the metric tail.  writes: id(node) -> ids of
    the variables whose gradients that node's backward writes.  buckets ({'lo', 'hi', 'vars'}):
    contiguous ranges of G, filled from the END of the Keras weight order (backward
    produces the last layers' gradients first); the metric tail rides in the first
    bucket.  A bucket is all-reduced on a side stream as soon as the backward ops that
    write its variables have been enqueued.  The bucket of the FIRST
    layers (written last, its all-reduce trails the whole backward) is cut at
    ``last_mb``, so the exposed tail of the step is one small all-reduce."""
    writers = {}
    for nd in plan.live:
        l = nd.layer
        if nd.kind in ("Conv2D", "Dense"):
            vs = [l.kernel] + ([l.bias] if l.use_bias else [])
            writers[id(nd)] = vs
        elif nd.kind == "DepthwiseConv2D":
            writers[id(nd)] = [l.depthwise_kernel] + ([l.bias] if l.use_bias else [])
        elif nd.kind == "BatchNormalization" and not nd.attrs.get("stats_only"):
            writers[id(nd)] = [w for w in (l.gamma, l.beta) if w is not None]
        elif nd.kind == "Add" and nd.attrs.get("fused"):
            main, (mode, other) = nd.attrs["fused"]
            vs = [w for w in (main.layer.gamma, main.layer.beta) if w is not None]
            if mode == "bn":
                vs += [w for w in (other.layer.gamma, other.layer.beta) if w is not None]
            writers[id(nd)] = vs
    writes = {k: [id(v) for v in vs] for k, vs in writers.items()}
    limit = max(1, int(bucket_mb * 2**20 / 4))
    first = []  # the first layers' variables, up to last_mb (reduced last)
    n_first, lim_first = 0, max(1, int(min(last_mb, bucket_mb) * 2**20 / 4))
    for i in range(len(variables)):
        if first and n_first + sizes[i] > lim_first:
            break
        first.append(i)
        n_first += sizes[i]
    order = list(range(len(first), len(variables)))[::-1]
    groups, cur, cur_n = [], [], 0
    for i in order:
        cur.append(i)
        cur_n += sizes[i]
        if cur_n >= limit:
            groups.append(cur)
            cur, cur_n = [], 0
    if cur:
        groups.append(cur)
    if first:
        groups.append(first)
    buckets = []
    for bi, idxs in enumerate(groups):
        lo = min(offsets[i] for i in idxs)
        hi = max(offsets[i] + sizes[i] for i in idxs)
        hi = _pad8(hi)
        if bi == 0:
            hi = total_elems  # + metric tail
        buckets.append({"lo": lo, "hi": hi, "vars": {id(variables[i]) for i in idxs}})
    # buckets must tile the buffer exactly
    spans = sorted((b["lo"], b["hi"]) for b in buckets)
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), spans
    return buckets, writes
