"""Learning-rate schedules (tf.keras.optimizers.schedules): pure functions of the optimizer's
``iterations``.

``schedule(step)`` takes the integer step -- the optimizer's ``iterations`` BEFORE the
update, so the first update uses ``schedule(0)`` (optimizer_v2 ``_decayed_lr``) -- and
returns a Python float evaluated in double precision.  All step logic (the staircase floor,
the cycle ceil, the clamps, the boundary search, the warm-up branch) is integer arithmetic.
The generic engine calls the schedule from ``apply_flat``; the native graph engine evaluates
the five classes below inside its optimizer kernel from the device-side iteration count
(ops/hip.py ``lr_table``; ops/reference.py ``lr_schedule32`` is that kernel's host mirror).
"""
from __future__ import annotations

import math


def _steps(v, what, low=1):
    """``v`` as given when it is a number >= low (an integral float becomes an int)."""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number, got {v!r}") from None
    if not f >= low:  # NaN included
        raise ValueError(f"{what} must be {'positive' if low > 0 else '>= %d' % low}, got {v!r}")
    return int(f) if f == int(f) else f


class LearningRateSchedule:
    """Base class: subclasses implement ``__call__(step)`` and ``get_config()``."""

    def __call__(self, step):
        raise NotImplementedError

    def get_config(self):
        raise NotImplementedError

    @classmethod
    def from_config(cls, config):
        return cls(**config)

    def __repr__(self):
        try:
            return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in self.get_config().items())})"
        except NotImplementedError:
            return f"{type(self).__name__}()"


class ExponentialDecay(LearningRateSchedule):
    """``init * decay_rate ** (step / decay_steps)`` (the exponent floored when staircase)."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        self.initial_learning_rate = float(initial_learning_rate)
        self.decay_steps = _steps(decay_steps, "decay_steps")
        self.decay_rate = float(decay_rate)
        self.staircase = bool(staircase)
        self.name = name

    def __call__(self, step):
        step = int(step)
        p = step // self.decay_steps if self.staircase else step / self.decay_steps
        return float(self.initial_learning_rate * self.decay_rate ** p)

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps,
                "decay_rate": self.decay_rate, "staircase": self.staircase, "name": self.name}


class InverseTimeDecay(LearningRateSchedule):
    """``init / (1 + decay_rate * step / decay_steps)`` (the quotient floored when staircase)."""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None):
        self.initial_learning_rate = float(initial_learning_rate)
        self.decay_steps = _steps(decay_steps, "decay_steps")
        self.decay_rate = float(decay_rate)
        self.staircase = bool(staircase)
        self.name = name

    def __call__(self, step):
        step = int(step)
        p = step // self.decay_steps if self.staircase else step / self.decay_steps
        return float(self.initial_learning_rate / (1.0 + self.decay_rate * p))

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps,
                "decay_rate": self.decay_rate, "staircase": self.staircase, "name": self.name}


class PolynomialDecay(LearningRateSchedule):
    """``(init - end) * (1 - s / d) ** power + end``; s = min(step, decay_steps), d =
    decay_steps -- or, with ``cycle``, s = step and d = decay_steps * max(1, ceil(step /
    decay_steps))."""

    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=0.0001, power=1.0, cycle=False,
                 name=None):
        self.initial_learning_rate = float(initial_learning_rate)
        self.decay_steps = _steps(decay_steps, "decay_steps")
        self.end_learning_rate = float(end_learning_rate)
        self.power = float(power)
        self.cycle = bool(cycle)
        self.name = name

    def __call__(self, step):
        step = int(step)
        if self.cycle:
            s, d = step, self.decay_steps * max(1, math.ceil(step / self.decay_steps))
        else:
            s, d = min(step, self.decay_steps), self.decay_steps
        return float((self.initial_learning_rate - self.end_learning_rate) * (1.0 - s / d) ** self.power
                     + self.end_learning_rate)

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps,
                "end_learning_rate": self.end_learning_rate, "power": self.power, "cycle": self.cycle,
                "name": self.name}


class PiecewiseConstantDecay(LearningRateSchedule):
    """``values[0]`` while step <= boundaries[0], ``values[i]`` while boundaries[i - 1] < step
    <= boundaries[i], ``values[-1]`` beyond the last boundary."""

    def __init__(self, boundaries, values, name=None):
        boundaries, values = list(boundaries), list(values)
        if len(values) != len(boundaries) + 1:
            raise ValueError(f"PiecewiseConstantDecay: {len(boundaries)} boundaries need {len(boundaries) + 1} "
                             f"values, got {len(values)}")
        bs = []
        for b in boundaries:
            f = float(b)
            bs.append(int(f) if f == int(f) else f)
        if any(b1 <= b0 for b0, b1 in zip(bs, bs[1:])):
            raise ValueError(f"PiecewiseConstantDecay: boundaries must strictly increase, got {boundaries!r}")
        self.boundaries = bs
        self.values = [float(v) for v in values]
        self.name = name

    def __call__(self, step):
        step = int(step)
        i = 0
        while i < len(self.boundaries) and step > self.boundaries[i]:
            i += 1
        return self.values[i]

    def get_config(self):
        return {"boundaries": list(self.boundaries), "values": list(self.values), "name": self.name}


class CosineDecay(LearningRateSchedule):
    """``init * ((1 - alpha) * 0.5 * (1 + cos(pi * s / decay_steps)) + alpha)``, s = min(step,
    decay_steps).  With a ``warmup_target``: linear from init to the target over
    ``warmup_steps`` steps, then the cosine from the target, counted from ``warmup_steps``."""

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0, name=None, warmup_target=None, warmup_steps=0):
        self.initial_learning_rate = float(initial_learning_rate)
        self.decay_steps = _steps(decay_steps, "decay_steps")
        self.alpha = float(alpha)
        self.name = name
        self.warmup_target = None if warmup_target is None else float(warmup_target)
        self.warmup_steps = _steps(warmup_steps, "warmup_steps", low=0)

    def _cosine(self, init, step):
        s = min(step, self.decay_steps)
        return init * ((1.0 - self.alpha) * 0.5 * (1.0 + math.cos(math.pi * s / self.decay_steps)) + self.alpha)

    def __call__(self, step):
        step = int(step)
        if self.warmup_target is None:
            return float(self._cosine(self.initial_learning_rate, step))
        if step < self.warmup_steps:
            return float(self.initial_learning_rate
                         + (self.warmup_target - self.initial_learning_rate) * step / self.warmup_steps)
        return float(self._cosine(self.warmup_target, step - self.warmup_steps))

    def get_config(self):
        return {"initial_learning_rate": self.initial_learning_rate, "decay_steps": self.decay_steps,
                "alpha": self.alpha, "name": self.name, "warmup_target": self.warmup_target,
                "warmup_steps": self.warmup_steps}


_CLASSES = {c.__name__: c for c in (ExponentialDecay, InverseTimeDecay, PolynomialDecay, PiecewiseConstantDecay,
                                    CosineDecay)}


def serialize(schedule):
    return {"class_name": type(schedule).__name__, "config": schedule.get_config()}


def deserialize(config, custom_objects=None):
    if isinstance(config, LearningRateSchedule):
        return config
    classes = dict(_CLASSES)
    classes.update(custom_objects or {})
    name = config["class_name"]
    if name not in classes:
        raise ValueError(f"unknown learning-rate schedule {name!r}")
    return classes[name].from_config(dict(config.get("config", {})))
