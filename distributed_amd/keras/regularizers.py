"""``tf.keras.regularizers``: weight penalties added to the training loss.

A regularizer is a callable ``w -> scalar``; a layer calls it on a variable (kernel, bias,
gamma, beta) and the engines add the result to the step's loss and its gradient to the
variable's gradient.  :class:`L1L2` is the closed form every engine implements directly
(``l1 * sum|w| + l2 * sum(w^2)``, gradient ``l1 * sign(w) + 2 * l2 * w`` with
``sign(0) = 0``); any other callable is differentiated by autograd on the generic engine.
"""
from __future__ import annotations

import torch


class Regularizer:
    def __call__(self, w):
        return torch.zeros((), dtype=torch.float32)

    def get_config(self) -> dict:
        return {}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class L1L2(Regularizer):
    def __init__(self, l1=0.0, l2=0.0):
        self.l1 = float(l1 or 0.0)
        self.l2 = float(l2 or 0.0)

    def __call__(self, w):
        w = torch.as_tensor(w)
        out = torch.zeros((), dtype=w.dtype, device=w.device)
        if self.l1:
            out = out + self.l1 * w.abs().sum()
        if self.l2:
            out = out + self.l2 * (w * w).sum()
        return out

    def get_config(self):
        return {"l1": self.l1, "l2": self.l2}

    def __repr__(self):
        return f"L1L2(l1={self.l1}, l2={self.l2})"


def l1(l=0.01):  # noqa: E741  (the Keras argument name)
    return L1L2(l1=l)


def l2(l=0.01):  # noqa: E741
    return L1L2(l2=l)


def l1_l2(l1=0.01, l2=0.01):
    return L1L2(l1=l1, l2=l2)


_CLASSES = {"L1L2": L1L2, "Regularizer": Regularizer}
_NAMES = {"l1": l1, "l2": l2, "l1_l2": l1_l2}


def serialize(reg):
    """The Keras config entry of a regularizer: ``{"class_name", "config"}`` or None."""
    if reg is None:
        return None
    if not isinstance(reg, Regularizer):
        raise ValueError(f"cannot serialize regularizer {name_of(reg)!r}: not a keras Regularizer")
    return {"class_name": type(reg).__name__, "config": reg.get_config()}


def deserialize(config):
    cls = _CLASSES.get(config["class_name"])
    if cls is None:
        raise ValueError(f"unknown regularizer class {config['class_name']!r}")
    return cls.from_config(dict(config.get("config") or {}))


def get(identifier):
    if identifier is None or isinstance(identifier, Regularizer):
        return identifier
    if isinstance(identifier, dict):
        return deserialize(identifier)
    if isinstance(identifier, str):
        fn = _NAMES.get(identifier)
        if fn is None:
            raise ValueError(f"unknown regularizer {identifier!r}")
        return fn()
    if callable(identifier):
        return identifier
    raise ValueError(f"cannot interpret regularizer {identifier!r}")


def name_of(reg) -> str:
    """A printable name of a regularizer (engine-selection reasons)."""
    return getattr(reg, "__name__", None) or type(reg).__name__


def coefficients(reg):
    """(l1, l2) of an :class:`L1L2`, or None for any other callable."""
    if isinstance(reg, L1L2):
        return reg.l1, reg.l2
    return None


def regularized(variables):
    """[(variable, regularizer)] of the variables that carry one."""
    return [(v, v.regularizer) for v in variables if getattr(v, "regularizer", None) is not None]


def penalty(variables) -> float:
    """R = sum of the regularizers of ``variables`` at their current values (host float)."""
    tot = 0.0
    with torch.no_grad():
        for v, r in regularized(variables):
            tot += float(r(v.value.detach()))
    return tot
