"""Keras backend utilities: layer-name uids, clear_session, floatx."""
from __future__ import annotations

import collections
import re

_UIDS = collections.defaultdict(int)


def get_uid(prefix: str) -> int:
    _UIDS[prefix] += 1
    return _UIDS[prefix]


def unique_name(prefix: str) -> str:
    """Keras naming: first 'dense', then 'dense_1', 'dense_2', ..."""
    n = get_uid(prefix)
    return prefix if n == 1 else f"{prefix}_{n - 1}"


def clear_session() -> None:
    _UIDS.clear()


def to_snake_case(name: str) -> str:
    s = re.sub(r"(.)([A-Z][a-z]+)", r"\1_\2", name)
    s = re.sub(r"([a-z])([A-Z])", r"\1_\2", s).lower()
    return s if s[0] != "_" else "private" + s


class AugmentContext:
    """What the input-augmentation layers draw from during a training step: the step ``t``
    (the optimizer's iterations + 1), the global batch slot of every row of the replica's
    batch, and the layers' effective seeds ({id(layer): seed}, keras/layers.py
    augment_seeds).  An engine sets it around the model's forward call."""

    def __init__(self, t: int, slots, seeds=None):
        self.t, self.slots, self.seeds = int(t), slots, dict(seeds or {})

    def __enter__(self):
        global _AUGMENT
        self._prev, _AUGMENT = _AUGMENT, self
        return self

    def __exit__(self, *exc):
        global _AUGMENT
        _AUGMENT = self._prev
        return False


_AUGMENT = None


def augment_context():
    """The active :class:`AugmentContext`, or None (a bare ``layer(x, training=True)``)."""
    return _AUGMENT


def floatx() -> str:
    return "float32"


def image_data_format() -> str:
    return "channels_last"
