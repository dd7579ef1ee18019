"""A torch fp32 re-execution of a lowered native plan (engine/native_plan.py ``lower``) on
any device, rounding at the plan's storage points: every planned tensor is bf16 (value and
gradient), the weights enter the convolutions / GEMMs as their bf16 shadow with a
straight-through gradient, the logits are fp32 with a bf16 gradient.  ``quantize=False`` is the
same walk without any rounding: the plain fp32 step.

Covers the node kinds of the depthwise / separable test models: Conv2D, DepthwiseConv2D,
BatchNormalization (batch statistics, or the moving ones with ``training=False``), ReLU /
Activation('relu'), GlobalAveragePooling2D and Dense, with linear or ReLU activations."""
import numpy as np
import torch

from distributed_amd.ops import reference as ref

from test_native_graph_gpu import _Q, _QG, _QW


def _ident(t):
    return t


def _act(layer, z):
    name = getattr(getattr(layer, "activation", None), "__name__", "linear")
    if name == "relu":
        return torch.relu(z)
    if name != "linear":
        raise NotImplementedError(f"plan walker: activation {name}")
    return z


def logits_of(plan, leaves, x, quantize=True, training=True):
    """The fp32 logits of ``plan`` for the batch x (numpy NHWC); leaves: {id(variable): tensor}."""
    Q, QW, QG = (_Q.apply, _QW.apply, _QG.apply) if quantize else (_ident, _ident, _ident)
    vals = {id(plan.x0.root()): Q(torch.from_numpy(np.asarray(x)).float())}

    def get(t):
        return vals[id(t.root())]

    logits = None
    for nd in plan.live:
        l, k = nd.layer, nd.kind
        if k == "Conv2D":
            w = leaves[id(l.kernel)]
            z = ref.conv2d(get(nd.inputs[0])[..., :w.shape[2]], QW(w), leaves[id(l.bias)] if l.use_bias else None,
                           l.strides, l.padding)
            out = Q(_act(l, z))
        elif k == "DepthwiseConv2D":
            z = ref.depthwise_conv2d(get(nd.inputs[0]), QW(leaves[id(l.depthwise_kernel)]),
                                     leaves[id(l.bias)] if l.use_bias else None, l.strides, l.padding)
            out = Q(_act(l, z))
        elif k == "BatchNormalization":
            xin = get(nd.inputs[0])
            if training:
                m, v = xin.mean(dim=(0, 1, 2)), xin.var(dim=(0, 1, 2), unbiased=False)
            else:
                m, v = l.moving_mean.value.detach().float().cpu(), l.moving_variance.value.detach().float().cpu()
            z = (xin - m) * torch.rsqrt(v + l.epsilon) * leaves[id(l.gamma)] + leaves[id(l.beta)]
            out = Q(torch.relu(z) if nd.attrs.get("relu") else z)
        elif k in ("ReLU", "Activation"):
            out = Q(torch.relu(get(nd.inputs[0])) if k == "ReLU" else _act(l, get(nd.inputs[0])))
        elif k == "GlobalAveragePooling2D":
            out = Q(get(nd.inputs[0]).mean(dim=(1, 2)))
        elif k == "Dense":
            z = get(nd.inputs[0]).reshape(len(x), -1) @ QW(leaves[id(l.kernel)])
            if l.use_bias:
                z = z + leaves[id(l.bias)]
            if nd.attrs.get("logits"):
                logits = QG(z)
                continue
            out = Q(_act(l, z))
        else:
            raise NotImplementedError(f"plan walker: node kind {k}")
        vals[id(nd.out.root())] = out
    return logits


def sgd_updates(plan, model, x, y, lr, quantize=True):
    """({id(variable): -lr * gradient}, loss) of one plain-SGD step of the mean sparse
    cross-entropy over the batch, from the model's current weights (on the CPU)."""
    leaves = {id(v): v.value.detach().float().cpu().clone().requires_grad_(True) for v in model.trainable_weights}
    logits = logits_of(plan, leaves, x, quantize)
    loss = ref.sparse_softmax_xent(logits, torch.from_numpy(np.asarray(y))).sum() / len(x)
    ids = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[i] for i in ids])
    return {i: -lr * g for i, g in zip(ids, grads)}, float(loss.detach())


def update_distance(d_a, d_b):
    """(relative error |a - b| / |b|, cosine) of two updates of one variable, in fp64."""
    a, b = d_a.double().ravel(), d_b.double().ravel()
    nb = b.norm().item()
    return (a - b).norm().item() / max(nb, 1e-30), float(a @ b) / max(a.norm().item() * nb, 1e-30)
