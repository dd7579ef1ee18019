"""DepthwiseConv2D / SeparableConv2D in the native planners (CPU, device-free): behind
DAMD_NATIVE_DEPTHWISE=1 the two layers plan natively -- eligibility, the two-node lowering of
the separable layer, the gradient-bucket writers, every rejection's reason -- and with the
switch unset or 0 nothing changes: the reasons of test_depthwise_api.py, the same ResNet plan."""
import numpy as np
import pytest
import torch

from distributed_amd import keras
from distributed_amd.engine.native_graph import NativeGraphEngine
from distributed_amd.engine.native_infer import NativeInference
from distributed_amd.engine.native_plan import SeparableDepthwise, SeparablePointwise, _act_name, lower, plan_buckets
from distributed_amd.models import resnet18

from test_depthwise_api import _model

L = keras.layers


class FakeGPUStrategy:
    device = torch.device("cuda")


def _compiled(m):
    m.compile(optimizer=keras.optimizers.SGD(0.1), loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True),
              metrics=["accuracy"])
    return m


def _one_separable():
    keras.backend.clear_session()
    return _compiled(keras.Sequential([L.SeparableConv2D(8, 3, input_shape=(8, 8, 8)), L.GlobalAveragePooling2D(),
                                       L.Dense(4)]))


def _around(make, cin=8):
    """The layer of ``make`` on ``cin`` channels: behind a Conv2D, or (a channel count no native
    Conv2D produces) as the first layer."""
    keras.backend.clear_session()
    if cin % 8:
        head = [make(input_shape=(8, 8, cin))]
    else:
        head = [L.Conv2D(cin, 3, padding="same", input_shape=(8, 8, 3)), make()]
    return _compiled(keras.Sequential(head + [L.GlobalAveragePooling2D(), L.Dense(4)]))


def _eligible_everywhere(m):
    return [NativeGraphEngine.eligible(m, FakeGPUStrategy()), NativeInference.eligible(m, "cuda"),
            NativeInference.eligible(m, "cuda", evaluate=True)]


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setenv("DAMD_NATIVE_DEPTHWISE", "1")


def test_both_models_are_eligible_with_the_switch(on):
    assert _eligible_everywhere(_compiled(_model())) == [(True, "")] * 3
    assert _eligible_everywhere(_one_separable()) == [(True, "")] * 3


@pytest.mark.parametrize("value", [None, "0"])
def test_without_the_switch_the_pinned_reasons_come_back(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("DAMD_NATIVE_DEPTHWISE", raising=False)
    else:
        monkeypatch.setenv("DAMD_NATIVE_DEPTHWISE", value)
    assert _eligible_everywhere(_compiled(_model())) == [(False, "layer DepthwiseConv2D")] * 3
    assert _eligible_everywhere(_one_separable()) == [(False, "layer SeparableConv2D")] * 3


def test_lowering_expands_the_separable_layer_into_two_nodes(on):
    m = _compiled(_model())
    conv, dw, sep, gap, dense = m.layers
    p = lower(m, 16)
    assert [nd.kind for nd in p.nodes] == ["Conv2D", "DepthwiseConv2D", "DepthwiseConv2D", "Conv2D",
                                           "GlobalAveragePooling2D", "Dense"]
    assert p.live == p.nodes
    n_dw, n_sd, n_sp = p.nodes[1:4]
    assert n_dw.layer is dw and n_dw.out.shape == (16, 8, 8, 8) and _act_name(n_dw.layer) == "relu"
    # the depthwise half: the layer's strides and padding, no bias, linear, onto the planned intermediate
    assert isinstance(n_sd.layer, SeparableDepthwise) and n_sd.layer.depthwise_kernel is sep.depthwise_kernel
    assert (n_sd.layer.kernel_size, n_sd.layer.strides, n_sd.layer.padding) == ((3, 3), (2, 2), "same")
    assert not n_sd.layer.use_bias and n_sd.layer.bias is None and _act_name(n_sd.layer) == "linear"
    assert n_sd.inputs == [n_dw.out] and n_sd.out.shape == (16, 4, 4, 8) and n_sd.out.dtype == torch.bfloat16
    assert n_sd.out.consumers == [n_sp] and n_sd.out.needs_grad
    # the pointwise half: a 1 x 1 'valid' Conv2D with the layer's bias and activation
    v = n_sp.layer
    assert isinstance(v, SeparablePointwise) and v.kernel is sep.pointwise_kernel and v.bias is sep.bias
    assert (v.kernel_size, v.strides, v.padding, v.dilation_rate) == ((1, 1), (1, 1), "valid", (1, 1))
    assert v.filters == 16 and v.use_bias and _act_name(v) == "relu"
    assert n_sp.inputs == [n_sd.out] and n_sp.out.shape == (16, 4, 4, 16)
    assert p.producer(n_sp.out) is n_sp and p.producer(n_sd.out) is n_sd
    with pytest.raises(AttributeError):
        v.kernel = None  # a read-only view
    # the inference plan is the same expansion
    assert [nd.kind for nd in lower(m, 16, inference=True).live] == [nd.kind for nd in p.live]


def test_pointwise_half_takes_the_conv_bn_statistics_fusion(on):
    keras.backend.clear_session()
    m = _compiled(keras.Sequential([
        L.Conv2D(8, 3, padding="same", activation="relu", input_shape=(8, 8, 3)),
        L.SeparableConv2D(16, 3, strides=2, padding="same", use_bias=False), L.BatchNormalization(), L.ReLU(),
        L.DepthwiseConv2D(3, padding="same"), L.BatchNormalization(), L.GlobalAveragePooling2D(), L.Dense(4)]))
    assert NativeGraphEngine.eligible(m, FakeGPUStrategy()) == (True, "")
    p = lower(m, 8)
    kinds = [nd.kind for nd in p.nodes]
    pw, bn1 = p.nodes[kinds.index("Conv2D", 1)], p.nodes[kinds.index("BatchNormalization")]
    assert pw.attrs.get("stats") and bn1.attrs.get("stats_from_conv") and bn1.attrs.get("relu")
    # a BatchNormalization behind a depthwise node keeps its own statistics pass
    bn2 = [nd for nd in p.nodes if nd.kind == "BatchNormalization"][1]
    assert p.producer(bn2.inputs[0]).kind == "DepthwiseConv2D" and not bn2.attrs.get("stats_from_conv")
    assert p.describe()["conv_bn_stats"] == 1


def test_bucket_writers_name_every_kernel_once_and_the_buckets_tile(on):
    m = _compiled(_model())
    p = lower(m, 16)
    vs = m.trainable_weights
    sizes = [int(np.prod(v.shape)) for v in vs]
    offsets, off = [], 0
    for sz in sizes:
        offsets.append(off)
        off = -(-(off + sz) // 8) * 8
    for mb in (1.0, 1e-4):  # one bucket; many
        buckets, writes = plan_buckets(p, vs, sizes, offsets, off + 8, mb, last_mb=mb)
        written = [i for ids in writes.values() for i in ids]
        assert sorted(written) == sorted(id(v) for v in vs)  # every variable, exactly once
        conv, dw, sep = m.layers[:3]
        n_dw, n_sd, n_sp = p.nodes[1:4]
        assert writes[id(n_dw)] == [id(dw.depthwise_kernel), id(dw.bias)]
        assert writes[id(n_sd)] == [id(sep.depthwise_kernel)]
        assert writes[id(n_sp)] == [id(sep.pointwise_kernel), id(sep.bias)]
        spans = sorted((b["lo"], b["hi"]) for b in buckets)
        assert spans[0][0] == 0 and spans[-1][1] == off + 8
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert sorted(i for b in buckets for i in b["vars"]) == sorted(id(v) for v in vs)
    assert len(buckets) > 1


REJECTED = [
    (lambda **kw: L.DepthwiseConv2D(3, depth_multiplier=2, **kw), 8, "depthwise depth_multiplier 2"),
    (lambda **kw: L.SeparableConv2D(8, 3, depth_multiplier=3, **kw), 8, "depthwise depth_multiplier 3"),
    (lambda **kw: L.DepthwiseConv2D(3, dilation_rate=2, **kw), 8, "depthwise geometry"),
    (lambda **kw: L.DepthwiseConv2D((3, 5), **kw), 8, "depthwise geometry"),
    (lambda **kw: L.DepthwiseConv2D(9, padding="same", **kw), 8, "depthwise geometry"),
    (lambda **kw: L.DepthwiseConv2D(3, strides=(1, 2), **kw), 8, "depthwise geometry"),
    (lambda **kw: L.SeparableConv2D(8, 3, strides=3, **kw), 8, "depthwise geometry"),
    (lambda **kw: L.DepthwiseConv2D(3, **kw), 12, "depthwise input channels must be a multiple of 8"),
    (lambda **kw: L.SeparableConv2D(8, 3, **kw), 12, "depthwise input channels must be a multiple of 8"),
    (lambda **kw: L.SeparableConv2D(12, 3, **kw), 8, "separable filters must be a multiple of 8"),
    (lambda **kw: L.DepthwiseConv2D(3, activation="elu", **kw), 8, "activation elu"),
    (lambda **kw: L.SeparableConv2D(8, 3, activation="softmax", **kw), 8, "activation softmax"),
    # the first failing condition is the one reported
    (lambda **kw: L.SeparableConv2D(12, 9, depth_multiplier=2, activation="elu", **kw), 12,
     "depthwise depth_multiplier 2"),
    (lambda **kw: L.SeparableConv2D(12, 9, activation="elu", **kw), 12, "depthwise geometry"),
]


@pytest.mark.parametrize("make,cin,reason", REJECTED,
                         ids=[f"{i}-{r[2].replace(' ', '_')}" for i, r in enumerate(REJECTED)])
def test_rejections_give_their_reason(on, make, cin, reason):
    m = _around(make, cin)
    assert _eligible_everywhere(m) == [(False, reason)] * 3


def test_seven_by_seven_stride_two_sigmoid_is_accepted(on):
    for make in (lambda: L.DepthwiseConv2D(7, strides=2, activation="sigmoid"),
                 lambda: L.SeparableConv2D(16, 5, activation="tanh", use_bias=False)):
        assert _eligible_everywhere(_around(make)) == [(True, "")] * 3


def test_resnet_plan_is_the_same_with_and_without_the_switch(monkeypatch):
    def describe():
        keras.backend.clear_session()
        m = _compiled(resnet18(classes=10, input_shape=(32, 32, 3)))
        p = lower(m, 32)
        return (NativeGraphEngine.eligible(m, FakeGPUStrategy()), p.describe(), [nd.kind for nd in p.nodes],
                [sorted((k, str(v)) for k, v in nd.attrs.items() if isinstance(v, (bool, int))) for nd in p.nodes],
                p.cin_pad, [nd.out.shape for nd in p.nodes])

    monkeypatch.delenv("DAMD_NATIVE_DEPTHWISE", raising=False)
    off = describe()
    monkeypatch.setenv("DAMD_NATIVE_DEPTHWISE", "1")
    assert describe() == off
    assert off[0] == (True, "") and off[1]["conv_bn_stats"] > 0
