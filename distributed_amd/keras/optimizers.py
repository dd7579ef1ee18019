"""Keras optimizers (tf.keras 2.0 optimizer_v2 update rules) over flat fp32 buffers.

``SGD(learning_rate=0.001)`` is the reference optimizer (reference README.md:72, 302).
Master weights are always fp32 (an lr=1e-3 update is below bf16 resolution for most
weights).  ``apply_flat`` is the generic-engine update; the
fused ConvNet engine applies the same SGD/momentum rule inside its HIP kernels.
"""
from __future__ import annotations

import math

import torch

from . import schedules
from .schedules import LearningRateSchedule


CLIP_MODES = ("clipvalue", "clipnorm", "global_clipnorm")


class Optimizer:
    def __init__(self, learning_rate=0.001, name="Optimizer", **kw):
        if "lr" in kw:  # Keras alias
            learning_rate = kw.pop("lr")
        # a number, or a schedules.LearningRateSchedule evaluated at `iterations` every step
        self._lr = learning_rate if isinstance(learning_rate, LearningRateSchedule) else float(learning_rate)
        self._lr_listener = None  # weak method of the engine that mirrors the rate on a device
        # gradient clipping (tf.keras >= 2.4): at most one of clipvalue / clipnorm /
        # global_clipnorm, a finite number > 0.  Applied by the engines to the gradient the
        # update rule consumes (all-reduced mean gradient + weight-regularizer gradient), once
        # per step after the exchange; read when the engine is built (first fit).
        given = [(k, kw.pop(k)) for k in CLIP_MODES if kw.get(k) is not None]
        for k in CLIP_MODES:
            kw.pop(k, None)
        if len(given) > 1:
            raise ValueError(f"at most one of {', '.join(CLIP_MODES)} may be set, got "
                             f"{', '.join(k for k, _ in given)}")
        self.clipvalue = self.clipnorm = self.global_clipnorm = None
        for k, v in given:
            try:
                c = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"{k} must be a finite number > 0, got {v!r}") from None
            if not (math.isfinite(c) and c > 0.0):
                raise ValueError(f"{k} must be a finite number > 0, got {v!r}")
            setattr(self, k, c)
        self.name = name
        self._iterations = 0
        self._iter_source = None  # callable returning device-side iteration count
        self.slots = {}  # name -> flat fp32 tensor

    @property
    def learning_rate(self):
        return self._lr

    @learning_rate.setter
    def learning_rate(self, v):
        old, self._lr = self._lr, v if isinstance(v, LearningRateSchedule) else float(v)
        # a schedule coming or going changes what the native engine captured (a plain
        # number is picked up from ctrl at the next epoch, as ever)
        if isinstance(old, LearningRateSchedule) or isinstance(v, LearningRateSchedule):
            hook = self._lr_listener() if self._lr_listener is not None else None
            if hook is not None:
                hook()

    lr = learning_rate

    def current_lr(self, step=None) -> float:
        """The rate of the update at ``step`` (default: the current ``iterations``): the
        number given, or the schedule evaluated there."""
        if isinstance(self._lr, LearningRateSchedule):
            return float(self._lr(self._iterations if step is None else int(step)))
        return self._lr

    @property
    def iterations(self) -> int:
        if self._iter_source is not None:
            return int(self._iter_source())
        return self._iterations

    @iterations.setter
    def iterations(self, v):
        self._iterations = int(v)

    def slot_names(self):
        return []

    def ensure_slots(self, n: int, device):
        for s in self.slot_names():
            if s not in self.slots or self.slots[s].numel() != n or self.slots[s].device != device:
                self.slots[s] = torch.zeros(n, dtype=torch.float32, device=device)

    def apply_flat(self, p: torch.Tensor, g: torch.Tensor) -> None:
        raise NotImplementedError

    def clipping(self):
        """(mode, value) of the configured gradient clipping -- mode one of CLIP_MODES -- or
        (None, None).  The one place the engines ask."""
        for k in CLIP_MODES:
            v = getattr(self, k)
            if v is not None:
                return k, float(v)
        return None, None

    def get_config(self):
        lr = schedules.serialize(self._lr) if isinstance(self._lr, LearningRateSchedule) else self._lr
        c = {"name": self.name, "learning_rate": lr}
        mode, v = self.clipping()
        if mode is not None:  # only when set: configs without clipping are what they were
            c[mode] = v
        return c


class SGD(Optimizer):
    def __init__(self, learning_rate=0.01, momentum=0.0, nesterov=False, name="SGD", **kw):
        super().__init__(learning_rate, name, **kw)
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)

    def slot_names(self):
        return ["momentum"] if self.momentum else []

    @torch.no_grad()
    def apply_flat(self, p, g):
        lr = self.current_lr()
        if self.momentum == 0.0:
            p.add_(g, alpha=-lr)
        else:
            v = self.slots["momentum"]
            v.mul_(self.momentum).add_(g, alpha=-lr)
            if self.nesterov:
                p.add_(v, alpha=self.momentum).add_(g, alpha=-lr)
            else:
                p.add_(v)
        self._iterations += 1

    def get_config(self):
        c = super().get_config()
        c.update(decay=0.0, momentum=self.momentum, nesterov=self.nesterov)
        return c


class Adam(Optimizer):
    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, name="Adam",
                 **kw):
        super().__init__(learning_rate, name, **kw)
        self.beta_1, self.beta_2, self.epsilon, self.amsgrad = beta_1, beta_2, epsilon, amsgrad

    def slot_names(self):
        return ["m", "v"] + (["vhat"] if self.amsgrad else [])

    @torch.no_grad()
    def apply_flat(self, p, g):
        t = self._iterations + 1
        m, v = self.slots["m"], self.slots["v"]
        m.mul_(self.beta_1).add_(g, alpha=1 - self.beta_1)
        v.mul_(self.beta_2).addcmul_(g, g, value=1 - self.beta_2)
        lr_t = self.current_lr() * math.sqrt(1 - self.beta_2 ** t) / (1 - self.beta_1 ** t)
        if self.amsgrad:
            vh = self.slots["vhat"]
            torch.maximum(vh, v, out=vh)
            p.addcdiv_(m, vh.sqrt().add_(self.epsilon), value=-lr_t)
        else:
            p.addcdiv_(m, v.sqrt().add_(self.epsilon), value=-lr_t)
        self._iterations = t

    def get_config(self):
        c = super().get_config()
        c.update(decay=0.0, beta_1=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon, amsgrad=self.amsgrad)
        return c


class RMSprop(Optimizer):
    def __init__(self, learning_rate=0.001, rho=0.9, momentum=0.0, epsilon=1e-7, centered=False, name="RMSprop",
                 **kw):
        super().__init__(learning_rate, name, **kw)
        self.rho, self.momentum, self.epsilon, self.centered = rho, momentum, epsilon, centered

    def slot_names(self):
        return ["rms"] + (["momentum"] if self.momentum else []) + (["mg"] if self.centered else [])

    @torch.no_grad()
    def apply_flat(self, p, g):
        ms = self.slots["rms"]
        ms.mul_(self.rho).addcmul_(g, g, value=1 - self.rho)
        denom = ms
        if self.centered:
            mg = self.slots["mg"]
            mg.mul_(self.rho).add_(g, alpha=1 - self.rho)
            denom = ms - mg * mg
        upd = g / (denom.sqrt() + self.epsilon) * self.current_lr()
        if self.momentum:
            mom = self.slots["momentum"]
            mom.mul_(self.momentum).add_(upd)
            p.sub_(mom)
        else:
            p.sub_(upd)
        self._iterations += 1

    def get_config(self):
        c = super().get_config()
        c.update(decay=0.0, rho=self.rho, momentum=self.momentum, epsilon=self.epsilon, centered=self.centered)
        return c


_ALIASES = {"sgd": SGD, "adam": Adam, "rmsprop": RMSprop}
_CLASSES = {c.__name__: c for c in _ALIASES.values()}


def get(identifier) -> Optimizer:
    if isinstance(identifier, Optimizer):
        return identifier
    if isinstance(identifier, str):
        return _ALIASES[identifier.lower()]()
    if isinstance(identifier, dict):
        cfg = dict(identifier.get("config", {}))
        cfg.pop("decay", None)
        for k in ("learning_rate", "lr"):
            if isinstance(cfg.get(k), dict):
                cfg[k] = schedules.deserialize(cfg[k])
        return _CLASSES[identifier["class_name"]](**cfg)
    raise ValueError(f"unknown optimizer {identifier!r}")


def serialize(opt: Optimizer):
    return {"class_name": type(opt).__name__, "config": opt.get_config()}
