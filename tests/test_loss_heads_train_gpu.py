"""The loss heads of the native engines end to end: one-hot / smoothed categorical
cross-entropy and softmax outputs through fit, evaluate and predict, against the PyTorch
path (DAMD_NATIVE_GRAPH=0 / DAMD_NATIVE_INFER=0) and against the native sparse head.

The net is the 28x28x1 CNN of test_native_graph_gpu.py with the head under test."""
import os

import numpy as np
import pytest

import distributed_amd as tf
from distributed_amd.engine.native_infer import NativeInference
from distributed_amd.keras.utils import to_categorical

from test_native_graph_gpu import _compare_updates, _data

pytestmark = pytest.mark.gpu

L = tf.keras.layers
SCE, CCE = tf.keras.losses.SparseCategoricalCrossentropy, tf.keras.losses.CategoricalCrossentropy
NAMES = ["k", "b", "k1", "b1", "k2", "b2"]


def _net(head="linear"):
    tail = {"linear": [L.Dense(10)], "softmax": [L.Dense(10, activation="softmax")],
            "layer": [L.Dense(10), L.Softmax()]}[head]
    return tf.keras.Sequential([L.Conv2D(32, 3, activation="relu", input_shape=(28, 28, 1)), L.MaxPooling2D(),
                                L.Flatten(), L.Dense(64, activation="relu")] + tail)


class _Env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _fit(head, loss, x, y, init, steps=3, batch=32, native=True, lr=0.05, momentum=0.0, keep=False, **env):
    """(weights, history, engine name, model) of one short run from ``init``; ``keep``: the
    runtime stays up, so the model can go on to predict / evaluate."""
    from distributed_amd.parallel import runtime

    if native:
        e = {"DAMD_NATIVE_GRAPH": "1", "DAMD_FUSED": "0", "DAMD_STRICT_NATIVE": "1"}
    else:  # the PyTorch path in fp32, as the reference runs of test_native_graph_gpu.py
        e = {"DAMD_NATIVE_GRAPH": "0", "DAMD_FUSED": "0", "DAMD_DEVICE": "cpu"}
    e.update(env)
    with _Env(**e):
        runtime.shutdown()
        try:
            tf.keras.backend.clear_session()
            m = _net(head)
            m.compile(loss=loss() if callable(loss) else loss,
                      optimizer=tf.keras.optimizers.SGD(learning_rate=lr, momentum=momentum), metrics=["accuracy"])
            m.set_weights(init)
            h = m.fit(x, y, batch_size=batch, epochs=1, steps_per_epoch=steps, shuffle=False, verbose=0)
            return m.get_weights(), h.history, m._engine.name, m
        finally:
            if not keep:
                runtime.shutdown()


def _init():
    tf.keras.backend.clear_session()
    return _net().get_weights()


def test_smoothed_one_hot_cce_tracks_the_pytorch_path():
    x, y = _data(96, (28, 28, 1), 10, seed=21)
    yc = to_categorical(y, 10)
    init = _init()
    loss = lambda: CCE(from_logits=True, label_smoothing=0.1)  # noqa: E731
    # (DAMD_FUSED at its default: the MNIST CNN with this head lands on the native graph engine)
    wn, hn, en, _ = _fit("linear", loss, x, yc, init, DAMD_FUSED="1")
    wr, hr, er, _ = _fit("linear", loss, x, yc, init, native=False)
    assert en == "native_graph" and er == "generic"
    assert set(hn) == set(hr) == {"loss", "accuracy"}
    np.testing.assert_allclose(hn["loss"], hr["loss"], rtol=1e-2)
    np.testing.assert_allclose(hn["accuracy"], hr["accuracy"], atol=1.5 / 100)
    _compare_updates(init, wn, wr, NAMES)


@pytest.mark.parametrize("head", ["softmax", "layer"])
def test_softmax_output_with_the_string_loss_is_the_sparse_step(head):
    """Dense(10, activation='softmax') (or Dense + Softmax()) with the string loss launches
    exactly the kernels of the linear model with from_logits=True: the same bits."""
    x, y = _data(96, (28, 28, 1), 10, seed=22)
    init = _init()
    wp, hp, ep, _ = _fit(head, "sparse_categorical_crossentropy", x, y, init, momentum=0.9)
    wl, hl, el, _ = _fit("linear", lambda: SCE(from_logits=True), x, y, init, momentum=0.9)
    assert ep == el == "native_graph"
    for a, b in zip(wp, wl):
        np.testing.assert_array_equal(a, b)
    assert hp["loss"] == hl["loss"] and hp["accuracy"] == hl["accuracy"]


def test_one_hot_cce_equals_the_sparse_loss():
    x, y = _data(96, (28, 28, 1), 10, seed=23)
    init = _init()
    wd, hd, ed, _ = _fit("linear", lambda: CCE(from_logits=True), x, to_categorical(y, 10), init)
    ws, hs, es, _ = _fit("linear", lambda: SCE(from_logits=True), x, y, init)
    assert ed == es == "native_graph"
    for a, b in zip(wd, ws):
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(hd["loss"], hs["loss"], rtol=1e-5)
    assert hd["accuracy"] == hs["accuracy"]


def test_short_final_batch_with_dense_targets():
    """100 rows at batch 32: the fourth step has 4 real rows; the 28 rows past the end get
    no gradient, loss or metric and the step is scaled by 1/4."""
    x, y = _data(100, (28, 28, 1), 10, seed=24)
    yc = to_categorical(y, 10)
    init = _init()
    loss = lambda: CCE(from_logits=True, label_smoothing=0.1)  # noqa: E731
    wn, hn, en, _ = _fit("linear", loss, x, yc, init, steps=None)
    wr, hr, er, _ = _fit("linear", loss, x, yc, init, steps=None, native=False)
    assert en == "native_graph" and er == "generic"
    np.testing.assert_allclose(hn["loss"], hr["loss"], rtol=1e-2)
    np.testing.assert_allclose(hn["accuracy"], hr["accuracy"], atol=1.5 / 100)


def test_dense_head_graph_replay_equals_eager_and_repeats():
    x, y = _data(128, (28, 28, 1), 10, seed=25)
    yc = to_categorical(y, 10)
    init = _init()
    loss = lambda: CCE(label_smoothing=0.1)  # noqa: E731  (probabilities: the softmax head)
    wg, hg, eg, _ = _fit("softmax", loss, x, yc, init, steps=4, momentum=0.9, DAMD_GRAPH="1")
    we, he, _, _ = _fit("softmax", loss, x, yc, init, steps=4, momentum=0.9, DAMD_GRAPH="0")
    wa, ha, _, _ = _fit("softmax", loss, x, yc, init, steps=4, momentum=0.9, DAMD_GRAPH="1")
    assert eg == "native_graph"
    for g, e, a in zip(wg, we, wa):
        np.testing.assert_array_equal(g, e)
        np.testing.assert_array_equal(g, a)
    assert hg["loss"] == he["loss"] == ha["loss"]


def test_targets_of_the_wrong_width_are_refused():
    x, y = _data(64, (28, 28, 1), 10, seed=26)
    init = _init()
    with pytest.raises(ValueError, match=r"\(n, 10\)"):
        _fit("linear", lambda: CCE(from_logits=True), x, y, init, steps=1)  # class ids
    with pytest.raises(ValueError, match=r"\(n, 10\)"):
        _fit("linear", lambda: CCE(from_logits=True), x, to_categorical(y, 12), init, steps=1)


@pytest.mark.parametrize("head,loss,dense", [("softmax", "sparse_categorical_crossentropy", False),
                                             ("softmax", "categorical_crossentropy", True),
                                             ("linear", lambda: CCE(from_logits=True), True)])
def test_predict_and_evaluate(head, loss, dense):
    x, y = _data(1000, (28, 28, 1), 10, seed=27)
    yt = to_categorical(y, 10) if dense else y
    _, _, en, m = _fit(head, loss, x, yt, _init(), steps=3, lr=0.05, momentum=0.9, keep=True)
    assert en == "native_graph"

    def both(fn):
        with _Env(DAMD_NATIVE_INFER="0"):
            ref = fn()
        m.__dict__.pop("_infer_plans", None)
        with _Env(DAMD_NATIVE_INFER="1", DAMD_STRICT_NATIVE="1"):
            nat = fn()
        assert any(isinstance(p, NativeInference) for p in m._infer_plans.values())
        return nat, ref

    nat, ref = both(lambda: m.predict(x, batch_size=128))  # 1000 = 7 x 128 + 104: a short last batch
    assert nat.shape == ref.shape == (1000, 10)
    assert np.abs(nat - ref).max() / (np.abs(ref).max() + 1e-9) < 3e-2
    if head == "softmax":
        assert np.abs(nat.sum(-1) - 1.0).max() < 1e-5
    nat, ref = both(lambda: m.evaluate(x, yt, batch_size=128, verbose=0, return_dict=True))
    assert set(nat) == set(ref) == {"loss", "accuracy"}
    assert abs(nat["loss"] - ref["loss"]) < 1e-2 * ref["loss"]
    assert abs(nat["accuracy"] - ref["accuracy"]) <= 5 / 1000
