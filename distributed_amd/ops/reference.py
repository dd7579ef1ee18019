"""Plain PyTorch reference ops in Keras (NHWC / HWIO) conventions.

Keras conventions reproduced (tf.keras 2.0 defaults, exercised by reference
README.md:58-73): channels_last activations ``[N,H,W,C]``, conv kernels ``[kh,kw,cin,cout]``,
dense kernels ``[in,out]``, 'valid'/'same' padding (TF 'same' pads the extra pixel at
the bottom/right), MaxPool ties resolved to the first max in row-major window order.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def _same_pad(in_size: int, k: int, s: int, d: int = 1):
    eff = (k - 1) * d + 1
    out = math.ceil(in_size / s)
    total = max((out - 1) * s + eff - in_size, 0)
    return total // 2, total - total // 2


def conv2d(x, w, b=None, strides=(1, 1), padding="valid", dilation=(1, 1)):
    """x [N,H,W,Cin], w [kh,kw,Cin,Cout] -> [N,Ho,Wo,Cout]."""
    xc = x.permute(0, 3, 1, 2)
    wc = w.permute(3, 2, 0, 1)
    if padding == "same":
        pt, pb = _same_pad(x.shape[1], w.shape[0], strides[0], dilation[0])
        pl, pr = _same_pad(x.shape[2], w.shape[1], strides[1], dilation[1])
        xc = F.pad(xc, (pl, pr, pt, pb))
    elif padding != "valid":
        raise ValueError(f"padding {padding!r}")
    y = F.conv2d(xc, wc, b, stride=tuple(strides), dilation=tuple(dilation))
    return y.permute(0, 2, 3, 1)


def depthwise_conv2d(x, w, b=None, strides=(1, 1), padding="valid", dilation=(1, 1)):
    """x [N,H,W,Cin], w [kh,kw,Cin,mult] -> [N,Ho,Wo,Cin*mult]: output channel c*mult + m is
    input channel c filtered by w[:, :, c, m] (TF's order: a grouped conv with groups = Cin
    over the kernel reshaped to [Cin*mult, 1, kh, kw])."""
    kh, kw, cin, mult = w.shape
    xc = x.permute(0, 3, 1, 2)
    wc = w.permute(2, 3, 0, 1).reshape(cin * mult, 1, kh, kw)
    if padding == "same":
        pt, pb = _same_pad(x.shape[1], kh, strides[0], dilation[0])
        pl, pr = _same_pad(x.shape[2], kw, strides[1], dilation[1])
        xc = F.pad(xc, (pl, pr, pt, pb))
    elif padding != "valid":
        raise ValueError(f"padding {padding!r}")
    y = F.conv2d(xc, wc, b, stride=tuple(strides), dilation=tuple(dilation), groups=cin)
    return y.permute(0, 2, 3, 1)


def maxpool2d(x, pool=(2, 2), strides=None, padding="valid"):
    strides = strides or pool
    xc = x.permute(0, 3, 1, 2)
    if padding == "same":
        pt, pb = _same_pad(x.shape[1], pool[0], strides[0])
        pl, pr = _same_pad(x.shape[2], pool[1], strides[1])
        xc = F.pad(xc, (pl, pr, pt, pb), value=float("-inf"))
    y = F.max_pool2d(xc, tuple(pool), tuple(strides))
    return y.permute(0, 2, 3, 1)


def avgpool2d(x, pool=(2, 2), strides=None, padding="valid"):
    strides = strides or pool
    xc = x.permute(0, 3, 1, 2)
    if padding == "same":
        # TF 'same' average pooling excludes the padding from the divisor
        pt, pb = _same_pad(x.shape[1], pool[0], strides[0])
        pl, pr = _same_pad(x.shape[2], pool[1], strides[1])
        ones = torch.ones_like(xc[:, :1])
        num = F.avg_pool2d(F.pad(xc, (pl, pr, pt, pb)), tuple(pool), tuple(strides), divisor_override=1)
        den = F.avg_pool2d(F.pad(ones, (pl, pr, pt, pb)), tuple(pool), tuple(strides), divisor_override=1)
        y = num / den
    else:
        y = F.avg_pool2d(xc, tuple(pool), tuple(strides))
    return y.permute(0, 2, 3, 1)


def dense(x, w, b=None):
    y = x.matmul(w)
    return y + b if b is not None else y


def batchnorm(x, gamma, beta, mean, var, training, momentum=0.99, eps=1e-3):
    """Keras BatchNormalization over the last axis; updates moving stats in place."""
    if training:
        dims = tuple(range(x.dim() - 1))
        bm = x.mean(dim=dims)
        bv = x.var(dim=dims, unbiased=False)
        with torch.no_grad():
            mean.mul_(momentum).add_(bm.detach(), alpha=1 - momentum)
            var.mul_(momentum).add_(bv.detach(), alpha=1 - momentum)
        m, v = bm, bv
    else:
        m, v = mean, var
    return (x - m) * torch.rsqrt(v + eps) * gamma + beta


def reg_grad(P, table):
    """fp32 gradient of the L1/L2 weight penalty over a flat buffer ``P``: for every row
    ``(offset, size, l1, l2)`` of ``table``, ``2 * l2 * w + l1 * sign(w)`` (sign(0) = 0) on
    ``P[offset:offset + size]``; zero elsewhere."""
    g = torch.zeros_like(P, dtype=torch.float32)
    for off, size, l1, l2 in table:
        w = P[int(off):int(off) + int(size)].float()
        g[int(off):int(off) + int(size)] = 2.0 * float(l2) * w + float(l1) * torch.sign(w)
    return g


def reg_penalty(P, table):
    """fp32 scalar ``R = sum over rows of l1 * sum|w| + l2 * sum(w^2)`` (rows as reg_grad)."""
    r = torch.zeros((), dtype=torch.float32, device=P.device)
    for off, size, l1, l2 in table:
        w = P[int(off):int(off) + int(size)].float()
        r = r + float(l1) * w.abs().sum() + float(l2) * (w * w).sum()
    return r


def clip_scale(norm: float, c: float) -> float:
    """``c / max(norm, c)`` in fp32: exactly 1.0 while ``norm <= c`` (0 included), NaN for a
    non-finite norm (as tf.clip_by_global_norm: the update is poisoned visibly)."""
    if not math.isfinite(norm):
        return float("nan")
    c32 = torch.tensor(float(c), dtype=torch.float32)
    return float(c32 / torch.maximum(torch.tensor(float(norm), dtype=torch.float32), c32))


@torch.no_grad()
def clip_grad(g, table, mode, c):
    """Keras gradient clipping of the flat fp32 gradient ``g`` in place.  ``table``: one
    ``(offset, size)`` row per variable (further columns are ignored).  ``mode``:
    ``"clipvalue"``: g <- min(max(g, -c), c) per element; ``"clipnorm"``: per variable
    g_v <- g_v * c / max(||g_v||, c); ``"global_clipnorm"``: g <- g * c / max(||g||, c) over
    all rows.  Norms are accumulated in fp64, the scales and products are fp32.  Returns
    ``(norms, scales)`` as fp64 / fp32 lists -- one entry per row, a single entry for the
    global mode, empty for clipvalue."""
    rows = [(int(r[0]), int(r[1])) for r in table]
    if mode == "clipvalue":
        for off, size in rows:
            g[off:off + size].clamp_(-float(c), float(c))
        return [], []
    sq = [float(g[off:off + size].double().pow(2).sum()) for off, size in rows]
    if mode == "global_clipnorm":
        norm = math.sqrt(sum(sq))
        s = clip_scale(norm, c)
        for off, size in rows:
            g[off:off + size].mul_(s)
        return [norm], [s]
    if mode != "clipnorm":
        raise ValueError(f"clip_grad: mode {mode!r}")
    norms = [math.sqrt(v) for v in sq]
    scales = [clip_scale(nv, c) for nv in norms]
    for (off, size), s in zip(rows, scales):
        g[off:off + size].mul_(s)
    return norms, scales


def lr_schedule32(schedule, step) -> float:
    """The fp32 host mirror of opt_step's device-side learning-rate schedule (optimizer.hip
    lr_eval): one of the five keras/schedules.py classes at the integer ``step``, the same
    operations in the same order in ``numpy.float32``, all step logic in integers.  Returns
    the float32 as a Python float."""
    import numpy as np

    f = np.float32
    step = max(int(step), 0)
    name = type(schedule).__name__
    if name == "PiecewiseConstantDecay":
        v = schedule.values[0]
        for i, b in enumerate(schedule.boundaries):
            if step > int(b):
                v = schedule.values[i + 1]
        return float(f(v))
    ds = int(schedule.decay_steps)
    init = f(schedule.initial_learning_rate)
    if name in ("ExponentialDecay", "InverseTimeDecay"):
        p = f(step // ds) if schedule.staircase else f(step) / f(ds)
        a = f(schedule.decay_rate)
        if name == "ExponentialDecay":
            return float(init * np.power(a, p, dtype=f))
        return float(init / (f(1) + a * p))
    if name == "PolynomialDecay":
        s, d = min(step, ds), ds
        if schedule.cycle:
            s, d = step, ds * max(1, (step + ds - 1) // ds)
        end = f(schedule.end_learning_rate)
        return float((init - end) * np.power(f(1) - f(s) / f(d), f(schedule.power), dtype=f) + end)
    if name != "CosineDecay":
        raise ValueError(f"lr_schedule32: no device form of {name}")
    if schedule.warmup_target is not None:
        ws, target = int(schedule.warmup_steps), f(schedule.warmup_target)
        if step < ws:
            return float(init + (target - init) * f(step) / f(ws))
        init, step = target, step - ws
    s = min(step, ds)
    c = np.cos(f(np.pi) * f(s) / f(ds), dtype=f)
    a = f(schedule.alpha)
    return float(init * ((f(1) - a) * f(0.5) * (f(1) + c) + a))


def sparse_softmax_xent(logits, labels, weights=None):
    """Per-sample loss of SparseCategoricalCrossentropy(from_logits=True); with ``weights``
    (one per row) each row's loss times its weight."""
    ls = F.cross_entropy(logits.float(), labels.long(), reduction="none")
    return ls if weights is None else ls * weights.to(ls.dtype)


def softmax_xent_dense(logits, targets, label_smoothing=0.0, weights=None):
    """Per-sample loss of CategoricalCrossentropy(from_logits=True, label_smoothing) against
    dense target rows: -(y' * log_softmax(z)).sum(-1), y' = y (1 - eps) + eps / K; with
    ``weights`` (one per row) each row's loss times its weight."""
    y = targets.float()
    if label_smoothing:
        y = y * (1.0 - label_smoothing) + label_smoothing / y.shape[-1]
    ls = -(y * torch.log_softmax(logits.float(), dim=-1)).sum(-1)
    return ls if weights is None else ls * weights.to(ls.dtype)


def categorical_accuracy(logits, targets):
    """Per-sample 0/1 of categorical accuracy (both argmaxes: ties -> first index)."""
    return (logits.argmax(dim=-1) == targets.argmax(dim=-1)).float()


def sparse_accuracy(logits, labels):
    """Per-sample 0/1 of sparse categorical accuracy (argmax ties -> first index)."""
    return (logits.argmax(dim=-1) == labels.long()).float()
