"""DepthwiseConv2D / SeparableConv2D in the Keras API (CPU): shapes, numerics against an
independent torch grouped convolution, TF's output-channel order, config / JSON / HDF5 round
trips, generic-engine training against a plain-torch SGD loop, regularizers and the R verbs."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_amd import keras, r_api
from distributed_amd.ops import reference

L = keras.layers
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tf_same(size, k, s):
    out = math.ceil(size / s)
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def _torch_depthwise(x, w, b, stride, padding):
    """x NHWC, w [kh, kw, Cin, mult]: F.conv2d(groups=Cin) on NCHW with explicit TF-same padding
    (the extra row / column at the bottom / right)."""
    kh, kw, cin, mult = w.shape
    xc = torch.as_tensor(x).permute(0, 3, 1, 2)
    if padding == "same":
        pt, pb = _tf_same(xc.shape[2], kh, stride)
        pl, pr = _tf_same(xc.shape[3], kw, stride)
        xc = F.pad(xc, (pl, pr, pt, pb))
    wt = torch.empty(cin * mult, 1, kh, kw)
    for c in range(cin):
        for m in range(mult):
            wt[c * mult + m, 0] = torch.as_tensor(w[:, :, c, m])
    y = F.conv2d(xc, wt, None if b is None else torch.as_tensor(b), stride=stride, groups=cin)
    return y.permute(0, 2, 3, 1)


GEOS = [(h, w, k, s, p) for (h, w) in ((9, 7), (8, 10)) for (k, s) in ((3, 1), (3, 2), (5, 2))
        for p in ("valid", "same")]


@pytest.mark.parametrize("h,w,k,s,p", GEOS)
def test_shapes_params_and_numerics(h, w, k, s, p):
    keras.backend.clear_session()
    rng = np.random.default_rng(h * 100 + k * 10 + s)
    cin, filters = 6, 10
    x = rng.normal(size=(2, h, w, cin)).astype(np.float32)
    ho = math.ceil(h / s) if p == "same" else (h - k) // s + 1
    wo = math.ceil(w / s) if p == "same" else (w - k) // s + 1

    dw = L.DepthwiseConv2D(k, strides=s, padding=p, bias_initializer="glorot_uniform", input_shape=(h, w, cin))
    assert [v.shape for v in dw.weights] == [(k, k, cin, 1), (cin,)]
    assert dw.count_params() == k * k * cin + cin
    assert dw.compute_output_shape((None, h, w, cin)) == (None, ho, wo, cin) == dw.output_shape
    y = dw(torch.as_tensor(x))
    assert tuple(y.shape) == (2, ho, wo, cin)
    kern, bias = dw.get_weights()
    want = _torch_depthwise(x, kern, bias, s, p)
    np.testing.assert_allclose(y.numpy(), want.numpy(), rtol=1e-5, atol=1e-5)

    sep = L.SeparableConv2D(filters, k, strides=s, padding=p, activation="relu", bias_initializer="glorot_uniform",
                            input_shape=(h, w, cin))
    assert [v.shape for v in sep.weights] == [(k, k, cin, 1), (1, 1, cin, filters), (filters,)]
    assert sep.count_params() == k * k * cin + cin * filters + filters
    assert sep.compute_output_shape((None, h, w, cin)) == (None, ho, wo, filters)
    y = sep(torch.as_tensor(x))
    dk, pk, b = sep.get_weights()
    mid = _torch_depthwise(x, dk, None, s, p)  # no bias, no activation between the halves
    want = torch.relu(F.conv2d(mid.permute(0, 3, 1, 2), torch.as_tensor(pk).permute(3, 2, 0, 1),
                               torch.as_tensor(b)).permute(0, 2, 3, 1))
    np.testing.assert_allclose(y.numpy(), want.numpy(), rtol=1e-5, atol=1e-5)


def test_depth_multiplier_channel_order():
    """Output channel c * mult + m is input channel c under kernel[:, :, c, m] (TF's order)."""
    keras.backend.clear_session()
    cin, mult = 3, 2
    dw = L.DepthwiseConv2D(1, depth_multiplier=mult, use_bias=False, input_shape=(4, 5, cin))
    assert dw.depthwise_kernel.shape == (1, 1, cin, mult) and dw.output_shape == (None, 4, 5, cin * mult)
    kern = np.zeros((1, 1, cin, mult), np.float32)
    for c in range(cin):
        for m in range(mult):
            kern[0, 0, c, m] = 10 * (c + 1) + m + 1  # a different constant per (c, m)
    dw.set_weights([kern])
    x = np.random.default_rng(0).normal(size=(2, 4, 5, cin)).astype(np.float32)
    y = dw(torch.as_tensor(x)).numpy()
    for c in range(cin):
        for m in range(mult):
            np.testing.assert_allclose(y[..., c * mult + m], x[..., c] * kern[0, 0, c, m], rtol=1e-6)
    # 3x3, multiplier 2 against the independent reference, and through the separable layer
    dw3 = L.DepthwiseConv2D(3, depth_multiplier=2, padding="same", strides=2, input_shape=(7, 6, cin))
    k3, b3 = dw3.get_weights()
    x = np.random.default_rng(1).normal(size=(2, 7, 6, cin)).astype(np.float32)
    np.testing.assert_allclose(dw3(torch.as_tensor(x)).numpy(), _torch_depthwise(x, k3, b3, 2, "same").numpy(),
                               rtol=1e-5, atol=1e-5)
    sep = L.SeparableConv2D(4, 3, depth_multiplier=2, input_shape=(7, 6, cin))
    assert [v.shape for v in sep.weights] == [(3, 3, cin, 2), (1, 1, cin * 2, 4), (4,)]
    np.testing.assert_allclose(
        reference.depthwise_conv2d(torch.as_tensor(x), torch.as_tensor(k3), None, (2, 2), "same").numpy(),
        _torch_depthwise(x, k3, None, 2, "same").numpy(), rtol=1e-5, atol=1e-5)


def _model(reg=None):
    keras.backend.clear_session()
    return keras.Sequential([
        L.Conv2D(8, 3, padding="same", activation="relu", input_shape=(8, 8, 3)),
        L.DepthwiseConv2D(3, padding="same", activation="relu", depthwise_regularizer=reg),
        L.SeparableConv2D(16, 3, strides=2, padding="same", activation="relu"),
        L.GlobalAveragePooling2D(),
        L.Dense(4)])


def test_config_round_trips(tmp_path):
    keras.backend.clear_session()
    dw = L.DepthwiseConv2D((3, 3), strides=2, padding="same", depth_multiplier=2, activation="relu",
                           depthwise_regularizer=keras.regularizers.l2(1e-3), use_bias=False)
    c = dw.get_config()
    for key in ("kernel_size", "strides", "padding", "data_format", "dilation_rate", "depth_multiplier", "activation",
                "use_bias", "depthwise_initializer", "bias_initializer", "depthwise_regularizer", "bias_regularizer",
                "activity_regularizer", "depthwise_constraint", "bias_constraint"):
        assert key in c, key
    assert c["depthwise_constraint"] is None and c["bias_constraint"] is None and c["activity_regularizer"] is None
    assert c["depth_multiplier"] == 2 and c["kernel_size"] == [3, 3] and c["strides"] == [2, 2]
    dw2 = L.DepthwiseConv2D.from_config(c)
    assert dw2.get_config() == c and dw2.depthwise_regularizer.l2 == 1e-3
    sep = L.SeparableConv2D(12, 5, padding="same", pointwise_regularizer="l1", activation="tanh")
    c = sep.get_config()
    for key in ("filters", "depth_multiplier", "depthwise_initializer", "pointwise_initializer", "bias_initializer",
                "depthwise_regularizer", "pointwise_regularizer", "bias_regularizer", "activity_regularizer",
                "depthwise_constraint", "pointwise_constraint", "bias_constraint"):
        assert key in c, key
    assert c["pointwise_constraint"] is None and c["filters"] == 12
    sep2 = L.SeparableConv2D.from_config(c)
    assert sep2.get_config() == c and sep2.pointwise_regularizer.l1 == 0.01

    m = _model()
    m.compile(optimizer="sgd", loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    m2 = keras.models.model_from_json(m.to_json())
    assert [type(l).__name__ for l in m2.layers] == [type(l).__name__ for l in m.layers]
    assert m2.layers[2].get_config() == m.layers[2].get_config()
    path = str(tmp_path / "dw.h5")
    m.save(path)
    m3 = keras.models.load_model(path)
    assert [w.name for w in m3.layers[1].weights] == [f"{m.layers[1].name}/depthwise_kernel:0",
                                                      f"{m.layers[1].name}/bias:0"]
    assert [w.name.split("/")[-1] for w in m3.layers[2].weights] == ["depthwise_kernel:0", "pointwise_kernel:0",
                                                                      "bias:0"]
    assert m.layers[1].name == "depthwise_conv2d" and m.layers[2].name == "separable_conv2d"
    for a, b in zip(m.get_weights(), m3.get_weights()):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()  # bitwise
    assert m3.layers[2].get_config() == m.layers[2].get_config()
    x = np.random.default_rng(0).random((4, 8, 8, 3)).astype(np.float32)
    np.testing.assert_array_equal(m.predict(x), m3.predict(x))


def test_generic_training_matches_plain_torch_sgd():
    """5 SGD steps on the generic engine (CPU) against autograd over the same weights."""
    lr, steps, bs = 0.05, 5, 8
    m = _model()
    m.compile(optimizer=keras.optimizers.SGD(lr), loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    rng = np.random.default_rng(5)
    x = rng.random((bs * steps, 8, 8, 3)).astype(np.float32)
    y = rng.integers(0, 4, bs * steps)
    w0 = m.get_weights()
    m.fit(x, y, batch_size=bs, epochs=1, shuffle=False, verbose=0)
    assert m._engine.name == "generic"
    got = m.get_weights()

    ws = [torch.tensor(w, requires_grad=True) for w in w0]
    ck, cb, dk, db, sdk, spk, sb, fk, fb = ws

    def nchw_conv(t, k_hwio, b, stride, pad_same, groups=1):
        kh, kw = k_hwio.shape[:2]
        if pad_same:
            pt, pb = _tf_same(t.shape[2], kh, stride)
            pl, pr = _tf_same(t.shape[3], kw, stride)
            t = F.pad(t, (pl, pr, pt, pb))
        if groups > 1:
            wt = k_hwio.permute(2, 3, 0, 1).reshape(groups, 1, kh, kw)  # multiplier 1
        else:
            wt = k_hwio.permute(3, 2, 0, 1)
        return F.conv2d(t, wt, b, stride=stride, groups=groups)

    for i in range(steps):
        xb = torch.as_tensor(x[i * bs:(i + 1) * bs]).permute(0, 3, 1, 2)
        yb = torch.as_tensor(y[i * bs:(i + 1) * bs]).long()
        t = torch.relu(nchw_conv(xb, ck, cb, 1, True))
        t = torch.relu(nchw_conv(t, dk, db, 1, True, groups=8))
        t = nchw_conv(t, sdk, None, 2, True, groups=8)
        t = torch.relu(nchw_conv(t, spk, sb, 1, False))
        logits = t.mean(dim=(2, 3)) @ fk + fb
        loss = F.cross_entropy(logits, yb)
        grads = torch.autograd.grad(loss, ws)
        with torch.no_grad():
            for w, g in zip(ws, grads):
                w -= lr * g
    for a, b, w in zip(got, ws, m.weights):
        np.testing.assert_allclose(a, b.detach().numpy(), rtol=1e-5, atol=1e-6, err_msg=w.name)
    assert any(np.abs(a - b).max() > 1e-4 for a, b in zip(got[2:5], w0[2:5]))  # the new kernels moved


def test_regularizer_on_depthwise_kernel_is_a_model_loss():
    m = _model(reg=keras.regularizers.l2(0.5))
    assert len(m.losses) == 1
    k = m.layers[1].depthwise_kernel
    assert k.regularizer is m.layers[1].depthwise_regularizer
    np.testing.assert_allclose(float(m.losses[0]), 0.5 * float((k.numpy().astype(np.float64) ** 2).sum()), rtol=1e-5)
    assert [id(v) for v, _ in m._regularized()] == [id(k)]
    keras.backend.clear_session()
    sep = L.SeparableConv2D(8, 3, depthwise_regularizer="l2", pointwise_regularizer="l1", input_shape=(6, 6, 4))
    assert len(sep.losses) == 2


def test_native_planners_name_the_layer_they_do_not_cover():
    """There is no native depthwise kernel: on a GPU such a model takes the generic engine,
    and the planners' reason names the layer."""
    from distributed_amd.engine.native_graph import NativeGraphEngine
    from distributed_amd.engine.native_infer import NativeInference

    class FakeGPUStrategy:
        device = torch.device("cuda")

    m = _model()
    m.compile(optimizer=keras.optimizers.SGD(0.1), loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    assert NativeGraphEngine.eligible(m, FakeGPUStrategy()) == (False, "layer DepthwiseConv2D")
    assert NativeInference.eligible(m, "cuda") == (False, "layer DepthwiseConv2D")
    keras.backend.clear_session()
    sep = keras.Sequential([L.SeparableConv2D(8, 3, input_shape=(8, 8, 8)), L.GlobalAveragePooling2D(), L.Dense(4)])
    sep.compile(optimizer="sgd", loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    assert NativeGraphEngine.eligible(sep, FakeGPUStrategy()) == (False, "layer SeparableConv2D")


def test_unsupported_constraints_warn():
    with pytest.warns(UserWarning, match="depthwise_constraint"):
        L.DepthwiseConv2D(3, depthwise_constraint=lambda w: w)


def test_r_verbs():
    keras.backend.clear_session()
    m = r_api.pipe(r_api.keras_model_sequential(),
                   lambda o: r_api.layer_depthwise_conv_2d(o, kernel_size=3, padding="same", depth_multiplier=2.0,
                                                           input_shape=r_api.c(8, 8, 4)),
                   lambda o: r_api.layer_separable_conv_2d(o, filters=16.0, kernel_size=r_api.c(3, 3), strides=2,
                                                           activation="relu"))
    a, b = m.layers
    assert type(a) is L.DepthwiseConv2D and a.depth_multiplier == 2 and a.output_shape == (None, 8, 8, 8)
    assert type(b) is L.SeparableConv2D and b.filters == 16 and b.strides == (2, 2)
    assert b.output_shape == (None, 3, 3, 16)
    # without a model the verb returns the layer
    assert type(r_api.layer_depthwise_conv_2d(kernel_size=3)) is L.DepthwiseConv2D
    ns = open(os.path.join(ROOT, "R", "NAMESPACE")).read()
    verbs = open(os.path.join(ROOT, "R", "R", "keras_verbs.R")).read()
    for verb in ("layer_depthwise_conv_2d", "layer_separable_conv_2d"):
        assert f"export({verb})" in ns, verb
        assert f"{verb} <- function(" in verbs and f".r()${verb}(" in verbs, verb
