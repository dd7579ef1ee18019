"""Keras layers (tf.keras 2.0 semantics) over torch tensors.

Layers used by the reference model (reference README.md:58-68, 292-298):
``Conv2D``, ``MaxPooling2D``, ``Flatten``, ``Dense`` — with Keras default arguments,
initializers, NHWC layout and auto-naming (``conv2d``, ``max_pooling2d``, ``flatten``,
``dense``, ``dense_1``).  The extra layers (BatchNormalization, Add, pooling variants,
ZeroPadding2D, Activation, Dropout, Reshape, Input) support the functional API and
ResNet-18 (BASELINE.json:10); RandomFlip / RandomCrop are the input augmentation of its
training recipe.
"""
from __future__ import annotations

import math
import warnings
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from . import activations as _act
from . import backend as K
from . import initializers as _init
from . import regularizers as _reg


def _pair(v):
    if isinstance(v, (list, tuple)):
        return tuple(int(a) for a in v)
    return (int(v), int(v))


def _current_device() -> torch.device:
    from ..parallel.strategy import get_strategy

    return get_strategy().device


class Variable:
    """A named model variable; storage may be relocated into a flat engine buffer."""

    def __init__(self, name: str, value: torch.Tensor, trainable: bool = True, aggregation: str = "none",
                 regularizer=None):
        self.name = name
        self._t = value
        self.trainable = trainable
        # the weight penalty of this variable (keras/regularizers.py) or None: the engines add
        # regularizer(value) to the loss and its gradient to the variable's gradient
        self.regularizer = regularizer
        # tf.VariableAggregation of a mirrored variable read across replicas: "mean" marks
        # the SyncOnRead BN moving statistics (each replica updates its own copy, readers
        # see the replica mean), "none" variables are kept identical by construction
        self.aggregation = aggregation
        # weakref to the engine whose flat buffer holds this variable: host writes go
        # through its before/after hooks (flush a deferred update, refresh bf16 shadows)
        self._engine_ref = None

    @property
    def value(self) -> torch.Tensor:
        return self._t

    @property
    def shape(self):
        return tuple(self._t.shape)

    @property
    def dtype(self):
        return self._t.dtype

    def numpy(self) -> np.ndarray:
        return self._t.detach().to("cpu", torch.float32).numpy().copy()

    def assign(self, v) -> None:
        t = torch.as_tensor(np.asarray(v), dtype=self._t.dtype)
        if tuple(t.shape) != self.shape:
            raise ValueError(f"assign shape {tuple(t.shape)} != {self.shape} for {self.name}")
        eng = self._engine_ref() if self._engine_ref is not None else None
        if eng is not None:
            eng.before_external_write()
        with torch.no_grad():
            self._t.copy_(t.to(self._t.device))
        if eng is not None:
            eng.after_external_write()

    def _rebind(self, storage: torch.Tensor) -> None:
        """Point this variable at ``storage`` (same shape), copying the current value."""
        with torch.no_grad():
            storage.copy_(self._t.to(storage.device))
        self._t = storage

    def __repr__(self):
        return f"<Variable '{self.name}' shape={self.shape} dtype={self.dtype}>"


class KerasTensor:
    """Symbolic tensor of the functional API (shape excludes nothing: batch is None).

    ``node_index`` numbers the calls of ``layer`` (a layer applied twice owns two nodes):
    Keras' ``inbound_nodes`` / ``input_layers`` entries are ``[layer_name, node_index,
    tensor_index]``."""

    def __init__(self, shape, layer=None, inputs=None, node_index=0):
        self.shape = tuple(shape)
        self.layer = layer
        self.inputs = inputs or []
        self.node_index = node_index

    def __repr__(self):
        return f"<KerasTensor shape={self.shape}>"


# accepted for Keras compatibility and not applied: a non-None value warns
_UNSUPPORTED_KW = ("activity_regularizer", "kernel_constraint", "bias_constraint", "gamma_constraint",
                   "beta_constraint", "depthwise_constraint", "pointwise_constraint")


class Layer:
    def __init__(self, name: Optional[str] = None, input_shape=None, batch_input_shape=None, trainable=True,
                 dtype=None, **kwargs):
        for k in _UNSUPPORTED_KW:
            if kwargs.get(k) is not None:
                warnings.warn(f"{type(self).__name__}({k}=...) is not supported and has no effect", UserWarning,
                              stacklevel=3)
        self.name = name or K.unique_name(K.to_snake_case(type(self).__name__))
        self.trainable = trainable
        self.built = False
        self._weights: List[Variable] = []
        if batch_input_shape is not None:
            self._batch_input_shape = tuple(batch_input_shape)
        elif input_shape is not None:
            self._batch_input_shape = (None,) + tuple(int(d) for d in input_shape)
        else:
            self._batch_input_shape = None
        self.input_shape = None
        self.output_shape = None

    # --- weights -------------------------------------------------------------
    def add_weight(self, name, shape, initializer="zeros", trainable=True, aggregation="none",
                   regularizer=None) -> Variable:
        init = _init.get(initializer)
        val = init(tuple(shape)).to(torch.float32).to(_current_device())
        v = Variable(f"{self.name}/{name}:0", val, trainable, aggregation, _reg.get(regularizer))
        self._weights.append(v)
        return v

    @property
    def weights(self) -> List[Variable]:
        return self.trainable_weights + self.non_trainable_weights

    @property
    def trainable_weights(self) -> List[Variable]:
        return [w for w in self._weights if w.trainable and self.trainable]

    @property
    def non_trainable_weights(self) -> List[Variable]:
        return [w for w in self._weights if not (w.trainable and self.trainable)]

    def get_weights(self):
        return [w.numpy() for w in self.weights]

    def set_weights(self, values):
        ws = self.weights
        if len(values) != len(ws):
            raise ValueError(f"layer {self.name} expects {len(ws)} weights, got {len(values)}")
        for w, v in zip(ws, values):
            w.assign(v)

    def count_params(self) -> int:
        return int(sum(int(np.prod(w.shape)) for w in self.weights))

    @property
    def losses(self) -> List[torch.Tensor]:
        """The current weight-penalty scalars, one per regularized variable (a frozen
        layer's too, as in tf.keras)."""
        with torch.no_grad():
            return [r(v.value.detach()) for v, r in _reg.regularized(self._weights)]

    # --- build / call ----------------------------------------------------------
    def build(self, input_shape):
        self.built = True

    def _maybe_build(self, input_shape):
        if not self.built:
            self.input_shape = tuple(input_shape)
            self.build(tuple(input_shape))
            self.built = True
            self.output_shape = self.compute_output_shape(tuple(input_shape))

    def compute_output_shape(self, input_shape):
        return input_shape

    def call(self, x, training=False):
        raise NotImplementedError

    def __call__(self, x, training=False):
        if isinstance(x, KerasTensor) or (isinstance(x, (list, tuple)) and x and isinstance(x[0], KerasTensor)):
            ins = list(x) if isinstance(x, (list, tuple)) else [x]
            shp = [t.shape for t in ins] if isinstance(x, (list, tuple)) else x.shape
            self._maybe_build(shp)
            self._n_nodes = getattr(self, "_n_nodes", 0) + 1
            return KerasTensor(self.compute_output_shape(shp), self, ins, node_index=self._n_nodes - 1)
        shp = [tuple(t.shape) for t in x] if isinstance(x, (list, tuple)) else tuple(x.shape)
        self._maybe_build(shp)
        return self.call(x, training=training)

    def get_config(self) -> dict:
        cfg = {"name": self.name, "trainable": self.trainable, "dtype": "float32"}
        if self._batch_input_shape is not None:
            cfg["batch_input_shape"] = list(self._batch_input_shape)
        return cfg

    @classmethod
    def from_config(cls, config):
        return cls(**config)


class InputLayer(Layer):
    def __init__(self, input_shape=None, batch_size=None, name=None, sparse=False, **kw):
        super().__init__(name=name or K.unique_name("input"), input_shape=input_shape, **kw)

    def call(self, x, training=False):
        return x

    def get_config(self):
        return {"batch_input_shape": list(self._batch_input_shape), "dtype": "float32", "sparse": False,
                "name": self.name}


def Input(shape, batch_size=None, name=None):  # noqa: N802
    lyr = InputLayer(input_shape=tuple(shape), name=name)
    lyr._n_nodes = 1
    t = KerasTensor((batch_size,) + tuple(shape), lyr, [], node_index=0)
    lyr.built = True
    lyr.output_shape = t.shape
    return t


class Conv2D(Layer):
    def __init__(self, filters, kernel_size, strides=(1, 1), padding="valid", data_format=None, dilation_rate=(1, 1),
                 activation=None, use_bias=True, kernel_initializer="glorot_uniform", bias_initializer="zeros",
                 kernel_regularizer=None, bias_regularizer=None, **kw):
        super().__init__(**kw)
        self.kernel_regularizer = _reg.get(kernel_regularizer)
        self.bias_regularizer = _reg.get(bias_regularizer)
        if data_format not in (None, "channels_last"):
            raise ValueError("only channels_last (NHWC) is supported, as in the reference")
        self.filters = int(filters)
        self.kernel_size = _pair(kernel_size)
        self.strides = _pair(strides)
        self.padding = padding.lower()
        self.dilation_rate = _pair(dilation_rate)
        self.activation = _act.get(activation)
        self.use_bias = use_bias
        self.kernel_initializer = _init.get(kernel_initializer)
        self.bias_initializer = _init.get(bias_initializer)
        if self._batch_input_shape is not None:
            self._maybe_build(self._batch_input_shape)

    def build(self, input_shape):
        cin = int(input_shape[-1])
        self.kernel = self.add_weight("kernel", self.kernel_size + (cin, self.filters), self.kernel_initializer,
                                      regularizer=self.kernel_regularizer)
        self.bias = (self.add_weight("bias", (self.filters,), self.bias_initializer,
                                     regularizer=self.bias_regularizer) if self.use_bias else None)

    def compute_output_shape(self, s):
        n, h, w, _ = s
        out = []
        for size, k, st, d in zip((h, w), self.kernel_size, self.strides, self.dilation_rate):
            eff = (k - 1) * d + 1
            out.append(None if size is None else
                       (math.ceil(size / st) if self.padding == "same" else (size - eff) // st + 1))
        return (n, out[0], out[1], self.filters)

    def call(self, x, training=False):
        y = ops.conv2d(x, self.kernel.value, self.bias.value if self.bias is not None else None,
                       self.strides, self.padding, self.dilation_rate)
        return self.activation(y)

    def get_config(self):
        c = super().get_config()
        c.update(filters=self.filters, kernel_size=list(self.kernel_size), strides=list(self.strides),
                 padding=self.padding, data_format="channels_last", dilation_rate=list(self.dilation_rate),
                 activation=_act.serialize(self.activation), use_bias=self.use_bias,
                 kernel_initializer=_init.serialize(self.kernel_initializer),
                 bias_initializer=_init.serialize(self.bias_initializer),
                 kernel_regularizer=_reg.serialize(self.kernel_regularizer),
                 bias_regularizer=_reg.serialize(self.bias_regularizer), activity_regularizer=None,
                 kernel_constraint=None, bias_constraint=None)
        return c


class DepthwiseConv2D(Layer):
    """Keras DepthwiseConv2D: every input channel filtered on its own by ``depth_multiplier``
    kernels.  ``depthwise_kernel`` is ``(kh, kw, Cin, depth_multiplier)``; output channel
    ``c * depth_multiplier + m`` is input channel ``c`` under ``depthwise_kernel[:, :, c, m]``."""

    def __init__(self, kernel_size, strides=(1, 1), padding="valid", depth_multiplier=1, data_format=None,
                 dilation_rate=(1, 1), activation=None, use_bias=True, depthwise_initializer="glorot_uniform",
                 bias_initializer="zeros", depthwise_regularizer=None, bias_regularizer=None, **kw):
        super().__init__(**kw)
        self.depthwise_regularizer = _reg.get(depthwise_regularizer)
        self.bias_regularizer = _reg.get(bias_regularizer)
        if data_format not in (None, "channels_last"):
            raise ValueError("only channels_last (NHWC) is supported, as in the reference")
        self.kernel_size = _pair(kernel_size)
        self.strides = _pair(strides)
        self.padding = padding.lower()
        self.depth_multiplier = int(depth_multiplier)
        if self.depth_multiplier < 1:
            raise ValueError(f"depth_multiplier must be >= 1, got {depth_multiplier}")
        self.dilation_rate = _pair(dilation_rate)
        self.activation = _act.get(activation)
        self.use_bias = use_bias
        self.depthwise_initializer = _init.get(depthwise_initializer)
        self.bias_initializer = _init.get(bias_initializer)
        if self._batch_input_shape is not None:
            self._maybe_build(self._batch_input_shape)

    def _out_channels(self, cin):
        return cin * self.depth_multiplier

    def _build_depthwise(self, cin):
        self.depthwise_kernel = self.add_weight("depthwise_kernel", self.kernel_size + (cin, self.depth_multiplier),
                                                self.depthwise_initializer, regularizer=self.depthwise_regularizer)

    def build(self, input_shape):
        cin = int(input_shape[-1])
        self._build_depthwise(cin)
        self.bias = (self.add_weight("bias", (self._out_channels(cin),), self.bias_initializer,
                                     regularizer=self.bias_regularizer) if self.use_bias else None)

    def compute_output_shape(self, s):
        n, h, w, c = s
        out = []
        for size, k, st, d in zip((h, w), self.kernel_size, self.strides, self.dilation_rate):
            eff = (k - 1) * d + 1
            out.append(None if size is None else
                       (math.ceil(size / st) if self.padding == "same" else (size - eff) // st + 1))
        return (n, out[0], out[1], self._out_channels(c))

    def call(self, x, training=False):
        y = ops.depthwise_conv2d(x, self.depthwise_kernel.value, self.bias.value if self.bias is not None else None,
                                 self.strides, self.padding, self.dilation_rate)
        return self.activation(y)

    def get_config(self):
        c = super().get_config()
        c.update(kernel_size=list(self.kernel_size), strides=list(self.strides), padding=self.padding,
                 data_format="channels_last", dilation_rate=list(self.dilation_rate),
                 depth_multiplier=self.depth_multiplier, activation=_act.serialize(self.activation),
                 use_bias=self.use_bias, depthwise_initializer=_init.serialize(self.depthwise_initializer),
                 bias_initializer=_init.serialize(self.bias_initializer),
                 depthwise_regularizer=_reg.serialize(self.depthwise_regularizer),
                 bias_regularizer=_reg.serialize(self.bias_regularizer), activity_regularizer=None,
                 depthwise_constraint=None, bias_constraint=None)
        return c


class SeparableConv2D(DepthwiseConv2D):
    """Keras SeparableConv2D: a depthwise convolution (no bias, no activation) followed by a
    1x1 convolution over ``pointwise_kernel`` ``(1, 1, Cin * depth_multiplier, filters)``; bias
    and activation come after the pointwise half.  Weights in Keras order: depthwise_kernel,
    pointwise_kernel, bias."""

    def __init__(self, filters, kernel_size, strides=(1, 1), padding="valid", data_format=None,
                 dilation_rate=(1, 1), depth_multiplier=1, activation=None, use_bias=True,
                 depthwise_initializer="glorot_uniform", pointwise_initializer="glorot_uniform",
                 bias_initializer="zeros", depthwise_regularizer=None, pointwise_regularizer=None,
                 bias_regularizer=None, **kw):
        self.filters = int(filters)
        self.pointwise_initializer = _init.get(pointwise_initializer)
        self.pointwise_regularizer = _reg.get(pointwise_regularizer)
        super().__init__(kernel_size, strides=strides, padding=padding, depth_multiplier=depth_multiplier,
                         data_format=data_format, dilation_rate=dilation_rate, activation=activation,
                         use_bias=use_bias, depthwise_initializer=depthwise_initializer,
                         bias_initializer=bias_initializer, depthwise_regularizer=depthwise_regularizer,
                         bias_regularizer=bias_regularizer, **kw)

    def _out_channels(self, cin):
        return self.filters

    def build(self, input_shape):
        cin = int(input_shape[-1])
        self._build_depthwise(cin)
        self.pointwise_kernel = self.add_weight("pointwise_kernel",
                                                (1, 1, cin * self.depth_multiplier, self.filters),
                                                self.pointwise_initializer, regularizer=self.pointwise_regularizer)
        self.bias = (self.add_weight("bias", (self.filters,), self.bias_initializer,
                                     regularizer=self.bias_regularizer) if self.use_bias else None)

    def call(self, x, training=False):
        y = ops.depthwise_conv2d(x, self.depthwise_kernel.value, None, self.strides, self.padding,
                                 self.dilation_rate)
        y = ops.conv2d(y, self.pointwise_kernel.value, self.bias.value if self.bias is not None else None)
        return self.activation(y)

    def get_config(self):
        c = super().get_config()
        c.update(filters=self.filters, pointwise_initializer=_init.serialize(self.pointwise_initializer),
                 pointwise_regularizer=_reg.serialize(self.pointwise_regularizer), pointwise_constraint=None)
        return c


class _Pool2D(Layer):
    _op = None

    def __init__(self, pool_size=(2, 2), strides=None, padding="valid", data_format=None, **kw):
        super().__init__(**kw)
        self.pool_size = _pair(pool_size)
        self.strides = _pair(strides) if strides is not None else self.pool_size
        self.padding = padding.lower()

    def compute_output_shape(self, s):
        n, h, w, c = s
        out = []
        for size, k, st in zip((h, w), self.pool_size, self.strides):
            out.append(None if size is None else
                       (math.ceil(size / st) if self.padding == "same" else (size - k) // st + 1))
        return (n, out[0], out[1], c)

    def get_config(self):
        c = super().get_config()
        c.update(pool_size=list(self.pool_size), padding=self.padding, strides=list(self.strides),
                 data_format="channels_last")
        return c


class MaxPooling2D(_Pool2D):
    def call(self, x, training=False):
        return ops.maxpool2d(x, self.pool_size, self.strides, self.padding)


class AveragePooling2D(_Pool2D):
    def call(self, x, training=False):
        return ops.avgpool2d(x, self.pool_size, self.strides, self.padding)


MaxPool2D = MaxPooling2D
AvgPool2D = AveragePooling2D


class GlobalAveragePooling2D(Layer):
    def compute_output_shape(self, s):
        return (s[0], s[-1])

    def call(self, x, training=False):
        return x.mean(dim=(1, 2))

    def get_config(self):
        c = super().get_config()
        c["data_format"] = "channels_last"
        return c


class GlobalMaxPooling2D(GlobalAveragePooling2D):
    def call(self, x, training=False):
        return x.amax(dim=(1, 2))


class Flatten(Layer):
    def compute_output_shape(self, s):
        rest = s[1:]
        return (s[0], None if any(d is None for d in rest) else int(np.prod(rest)))

    def call(self, x, training=False):
        return x.reshape(x.shape[0], -1)  # NHWC row-major: Keras-compatible feature order

    def get_config(self):
        c = super().get_config()
        c["data_format"] = "channels_last"
        return c


class Reshape(Layer):
    def __init__(self, target_shape, **kw):
        super().__init__(**kw)
        self.target_shape = tuple(target_shape)

    def compute_output_shape(self, s):
        return (s[0],) + self.target_shape

    def call(self, x, training=False):
        return x.reshape((x.shape[0],) + self.target_shape)

    def get_config(self):
        c = super().get_config()
        c["target_shape"] = list(self.target_shape)
        return c


class Dense(Layer):
    def __init__(self, units, activation=None, use_bias=True, kernel_initializer="glorot_uniform",
                 bias_initializer="zeros", kernel_regularizer=None, bias_regularizer=None, **kw):
        super().__init__(**kw)
        self.kernel_regularizer = _reg.get(kernel_regularizer)
        self.bias_regularizer = _reg.get(bias_regularizer)
        self.units = int(units)
        self.activation = _act.get(activation)
        self.use_bias = use_bias
        self.kernel_initializer = _init.get(kernel_initializer)
        self.bias_initializer = _init.get(bias_initializer)
        if self._batch_input_shape is not None:
            self._maybe_build(self._batch_input_shape)

    def build(self, input_shape):
        fin = int(input_shape[-1])
        self.kernel = self.add_weight("kernel", (fin, self.units), self.kernel_initializer,
                                      regularizer=self.kernel_regularizer)
        self.bias = (self.add_weight("bias", (self.units,), self.bias_initializer,
                                     regularizer=self.bias_regularizer) if self.use_bias else None)

    def compute_output_shape(self, s):
        return tuple(s[:-1]) + (self.units,)

    def call(self, x, training=False):
        y = ops.dense(x, self.kernel.value, self.bias.value if self.bias is not None else None)
        return self.activation(y)

    def get_config(self):
        c = super().get_config()
        c.update(units=self.units, activation=_act.serialize(self.activation), use_bias=self.use_bias,
                 kernel_initializer=_init.serialize(self.kernel_initializer),
                 bias_initializer=_init.serialize(self.bias_initializer),
                 kernel_regularizer=_reg.serialize(self.kernel_regularizer),
                 bias_regularizer=_reg.serialize(self.bias_regularizer), activity_regularizer=None,
                 kernel_constraint=None, bias_constraint=None)
        return c


class Activation(Layer):
    def __init__(self, activation, **kw):
        super().__init__(**kw)
        self.activation = _act.get(activation)

    def call(self, x, training=False):
        return self.activation(x)

    def get_config(self):
        c = super().get_config()
        c["activation"] = _act.serialize(self.activation)
        return c


class ReLU(Layer):
    # the plain rectifier only: the options the engines' planners look at, at their Keras defaults
    max_value, negative_slope, threshold = None, 0.0, 0.0

    def call(self, x, training=False):
        return torch.relu(x)


class Softmax(Layer):
    def call(self, x, training=False):
        return torch.softmax(x, dim=-1)


class Dropout(Layer):
    def __init__(self, rate, noise_shape=None, seed=None, **kw):
        super().__init__(**kw)
        self.rate = float(rate)
        self.seed = seed

    def call(self, x, training=False):
        if not training or self.rate == 0.0:
            return x
        return torch.nn.functional.dropout(x, self.rate, training=True)

    def get_config(self):
        c = super().get_config()
        c.update(rate=self.rate, noise_shape=None, seed=self.seed)
        return c


class ZeroPadding2D(Layer):
    def __init__(self, padding=(1, 1), **kw):
        super().__init__(**kw)
        if isinstance(padding, int):
            padding = ((padding, padding), (padding, padding))
        elif isinstance(padding[0], int):
            padding = ((padding[0], padding[0]), (padding[1], padding[1]))
        self.padding = tuple(tuple(p) for p in padding)

    def compute_output_shape(self, s):
        (t, b), (l, r) = self.padding
        return (s[0], None if s[1] is None else s[1] + t + b, None if s[2] is None else s[2] + l + r, s[3])

    def call(self, x, training=False):
        (t, b), (l, r) = self.padding
        return torch.nn.functional.pad(x, (0, 0, l, r, t, b))

    def get_config(self):
        c = super().get_config()
        c["padding"] = [list(p) for p in self.padding]
        return c


class _RandomAugment(Layer):
    """Input augmentation drawn per sample from (effective seed, step t, global batch slot g)
    -- ops/hip.py aug_draws, the definition every engine shares: no RNG state, the same
    sample transform at any world size, and a resumed run continues the sequence.  t, g and
    the seed come from the engine's :class:`~backend.AugmentContext`; a bare
    ``layer(x, training=True)`` uses t = 1, g = 0 .. batch - 1 and the layer's own seed at
    position 0."""

    def _draw_args(self, x):
        from ..ops import hip as _hip

        ctx = K.augment_context()
        if ctx is None:
            return _hip.aug_seed(self.seed, 0), 1, np.arange(x.shape[0])
        seed = ctx.seeds.get(id(self), _hip.aug_seed(self.seed, 0))
        g = ctx.slots
        g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        if len(g) != x.shape[0]:
            raise ValueError(f"{type(self).__name__}: {len(g)} batch slots for {x.shape[0]} rows")
        return seed, ctx.t, g


class RandomFlip(_RandomAugment):
    """Keras RandomFlip.  Training: each sample is flipped left-right (``"horizontal"``)
    and / or up-down (``"vertical"``), each with probability 1/2, the two axes drawn
    independently.  Inference: identity."""

    def __init__(self, mode="horizontal_and_vertical", seed=None, **kw):
        super().__init__(**kw)
        if mode not in ("horizontal", "vertical", "horizontal_and_vertical"):
            raise ValueError(f"RandomFlip: mode must be 'horizontal', 'vertical' or 'horizontal_and_vertical', "
                             f"got {mode!r}")
        self.mode, self.seed = mode, seed

    def call(self, x, training=False):
        if not training:
            return x
        from ..ops import hip as _hip

        seed, t, g = self._draw_args(x)
        lr, ud = _hip.aug_flip_bits(seed, t, g, _hip.AUG_FLIP_MODES[self.mode])
        for bits, axis in ((lr, 2), (ud, 1)):
            if bits.any():
                m = torch.from_numpy(bits).to(x.device).view(-1, 1, 1, 1)
                x = torch.where(m, x.flip(axis), x)
        return x

    def get_config(self):
        c = super().get_config()
        c.update(mode=self.mode, seed=self.seed)
        return c


class RandomCrop(_RandomAugment):
    """Keras RandomCrop.  Training: each sample keeps a ``height`` x ``width`` window at an
    integer offset drawn per axis as a 32-bit hash reduced modulo the number of offsets
    (H - height + 1, W - width + 1) -- uniform up to the modulo's bias of at most range / 2^32.
    Inference: the centre window, at offsets (H - height) // 2 and (W - width) // 2.  An
    input smaller than the target raises ValueError when the layer is built (no resize)."""

    def __init__(self, height, width, seed=None, **kw):
        super().__init__(**kw)
        self.height, self.width, self.seed = int(height), int(width), seed
        if self.height < 1 or self.width < 1:
            raise ValueError(f"RandomCrop: height and width must be >= 1, got {height} x {width}")
        if self._batch_input_shape is not None:
            self._maybe_build(self._batch_input_shape)

    def build(self, input_shape):
        h, w = input_shape[1], input_shape[2]
        if (h is not None and h < self.height) or (w is not None and w < self.width):
            raise ValueError(f"RandomCrop({self.height}, {self.width}): the input {h} x {w} is smaller than the "
                             "target and there is no resize path")

    def compute_output_shape(self, s):
        return (s[0], self.height, self.width, s[3])

    def call(self, x, training=False):
        h, w = x.shape[1], x.shape[2]
        if h < self.height or w < self.width:
            raise ValueError(f"RandomCrop({self.height}, {self.width}): the input {h} x {w} is smaller than the target")
        if not training:
            oy, ox = (h - self.height) // 2, (w - self.width) // 2
            return x[:, oy:oy + self.height, ox:ox + self.width]
        from ..ops import hip as _hip

        seed, t, g = self._draw_args(x)
        oy, ox = _hip.aug_crop_offsets(seed, t, g, h - self.height + 1, w - self.width + 1)
        rows = torch.from_numpy(oy[:, None] + np.arange(self.height)[None, :]).to(x.device)
        cols = torch.from_numpy(ox[:, None] + np.arange(self.width)[None, :]).to(x.device)
        b = torch.arange(x.shape[0], device=x.device).view(-1, 1, 1)
        return x[b, rows[:, :, None], cols[:, None, :]]

    def get_config(self):
        c = super().get_config()
        c.update(height=self.height, width=self.width, seed=self.seed)
        return c


def augment_seeds(model) -> dict:
    """{id(layer): effective seed} of ``model``'s RandomFlip / RandomCrop layers: the layer's
    ``seed`` and its position among the model's layers (the input layer not counted) through
    ops/hip.py aug_seed -- the one definition every engine uses."""
    from ..ops import hip as _hip

    ls = [l for l in model.layers if not isinstance(l, InputLayer)]
    return {id(l): _hip.aug_seed(l.seed, i) for i, l in enumerate(ls) if isinstance(l, _RandomAugment)}


class BatchNormalization(Layer):
    """Keras BN over channels (axis=-1).  Under MWMS the batch statistics are per
    replica, as tf.keras 2.0's (non-synced) BatchNormalization; the moving
    statistics are SyncOnRead variables with MEAN aggregation (created inside
    ``strategy.scope()``, reference README.md:134-151): every replica updates its own
    copy and the model averages them across replicas at each epoch end (before
    validation, callbacks and checkpoints read them), so every worker holds, saves and
    evaluates with the replica mean."""

    def __init__(self, axis=-1, momentum=0.99, epsilon=1e-3, center=True, scale=True, beta_regularizer=None,
                 gamma_regularizer=None, **kw):
        super().__init__(**kw)
        self.axis, self.momentum, self.epsilon, self.center, self.scale = axis, momentum, epsilon, center, scale
        self.beta_regularizer = _reg.get(beta_regularizer)
        self.gamma_regularizer = _reg.get(gamma_regularizer)

    def build(self, input_shape):
        c = int(input_shape[-1])
        self.gamma = (self.add_weight("gamma", (c,), "ones", regularizer=self.gamma_regularizer)
                      if self.scale else None)
        self.beta = self.add_weight("beta", (c,), "zeros", regularizer=self.beta_regularizer) if self.center else None
        self.moving_mean = self.add_weight("moving_mean", (c,), "zeros", trainable=False, aggregation="mean")
        self.moving_variance = self.add_weight("moving_variance", (c,), "ones", trainable=False,
                                               aggregation="mean")

    def call(self, x, training=False):
        g = self.gamma.value if self.gamma is not None else torch.ones(x.shape[-1], device=x.device)
        b = self.beta.value if self.beta is not None else torch.zeros(x.shape[-1], device=x.device)
        return ops.batchnorm(x, g, b, self.moving_mean.value, self.moving_variance.value,
                             training and self.trainable, self.momentum, self.epsilon)

    def get_config(self):
        c = super().get_config()
        c.update(axis=self.axis, momentum=self.momentum, epsilon=self.epsilon, center=self.center,
                 scale=self.scale, beta_regularizer=_reg.serialize(self.beta_regularizer),
                 gamma_regularizer=_reg.serialize(self.gamma_regularizer))
        return c


class Add(Layer):
    def compute_output_shape(self, shapes):
        return tuple(shapes[0])

    def call(self, xs, training=False):
        out = xs[0]
        for t in xs[1:]:
            out = out + t
        return out


def add(inputs):
    return Add()(inputs)


LAYER_CLASSES = {c.__name__: c for c in (
    InputLayer, Conv2D, DepthwiseConv2D, SeparableConv2D, MaxPooling2D, AveragePooling2D, GlobalAveragePooling2D, GlobalMaxPooling2D, Flatten,
    Reshape, Dense, Activation, ReLU, Softmax, Dropout, ZeroPadding2D, RandomFlip, RandomCrop, BatchNormalization, Add)}
