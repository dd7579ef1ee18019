"""Loss heads of the native engines on CPU: which (output head, loss, metric) combinations
the planner accepts, why it rejects the rest, and how a softmax output is planned."""
import numpy as np

from distributed_amd import keras, r_api
from distributed_amd.engine.native_graph import NativeGraphEngine
from distributed_amd.engine.native_infer import NativeInference

L = keras.layers


class _FakeGPUStrategy:
    import torch as _t

    device = _t.device("cuda")


def _body():
    return [L.Conv2D(32, 3, activation="relu", input_shape=(28, 28, 1)), L.MaxPooling2D(), L.Flatten(),
            L.Dense(64, activation="relu")]


def _net(head):
    keras.backend.clear_session()
    tail = {"linear": [L.Dense(10)], "softmax": [L.Dense(10, activation="softmax")],
            "layer": [L.Dense(10), L.Softmax()], "activation": [L.Dense(10), L.Activation("softmax")],
            "middle": [L.Dense(16, activation="softmax"), L.Dense(10)],
            "middle_layer": [L.Dense(16), L.Softmax(), L.Dense(10)]}[head]
    return keras.Sequential(_body() + tail)


def _eligible(head, loss, metrics=("accuracy",)):
    m = _net(head)
    m.compile(loss=loss, optimizer=keras.optimizers.SGD(0.1), metrics=list(metrics))
    return NativeGraphEngine.eligible(m, _FakeGPUStrategy()), m


def test_accepted_heads():
    CCE, SCE = keras.losses.CategoricalCrossentropy, keras.losses.SparseCategoricalCrossentropy
    for head, loss, metrics in (
            ("softmax", "sparse_categorical_crossentropy", ["accuracy"]),
            ("layer", CCE(), ["accuracy"]),
            ("activation", CCE(label_smoothing=0.2), ["categorical_accuracy"]),
            ("linear", CCE(from_logits=True, label_smoothing=0.1), ["acc"]),
            ("linear", SCE(from_logits=True), ["sparse_categorical_accuracy"]),
            ("softmax", "categorical_crossentropy", [])):
        (ok, why), m = _eligible(head, loss, metrics)
        assert ok, (head, why)
        # evaluate and predict take the same decision from the same helper
        assert NativeInference.eligible(m, "cuda", evaluate=True) == (True, "")
        assert NativeInference.eligible(m, "cuda") == (True, "")


def test_rejections_say_why():
    CCE, SCE = keras.losses.CategoricalCrossentropy, keras.losses.SparseCategoricalCrossentropy
    cases = {
        "twice": ("softmax", SCE(from_logits=True), ["accuracy"]),
        "twice_layer": ("layer", CCE(from_logits=True), ["accuracy"]),
        "linear_probs": ("linear", CCE(), ["accuracy"]),
        "mse": ("linear", "mse", []),
        "bce": ("linear", keras.losses.BinaryCrossentropy(from_logits=True), []),
        "mae": ("linear", "mae", []),
        "metric": ("linear", CCE(from_logits=True), ["sparse_categorical_accuracy"]),
        "metric_sparse": ("linear", SCE(from_logits=True), ["categorical_accuracy"]),
        "middle": ("middle", SCE(from_logits=True), ["accuracy"]),
        "middle_layer": ("middle_layer", SCE(from_logits=True), ["accuracy"]),
    }
    why = {}
    for name, (head, loss, metrics) in cases.items():
        (ok, why[name]), m = _eligible(head, loss, metrics)
        assert not ok and why[name], name
        assert not NativeInference.eligible(m, "cuda", evaluate=True)[0], name
    assert "twice" in why["twice"] and "from_logits=True" in why["twice"]
    assert why["twice_layer"] == why["twice"]
    assert "from_logits=False" in why["linear_probs"] and "linear" in why["linear_probs"]
    assert why["mse"] == why["bce"] == why["mae"] == "loss"
    assert "sparse_categorical_accuracy" in why["metric"] and "CategoricalCrossentropy" in why["metric"]
    assert "categorical_accuracy" in why["metric_sparse"]
    assert "softmax" in why["middle"] and "Softmax" in why["middle_layer"]
    # the five kinds of rejection the planner names are told apart by the reason alone
    assert len({why[k] for k in ("twice", "linear_probs", "mse", "metric", "middle")}) == 5


def test_predict_eligibility_does_not_depend_on_the_loss():
    (ok, _), m = _eligible("softmax", "mse", [])
    assert not ok
    assert NativeInference.eligible(m, "cuda") == (True, "")
    assert not NativeInference.eligible(m, "cuda", evaluate=True)[0]
    (_, _), m = _eligible("middle", "mse", [])
    assert not NativeInference.eligible(m, "cuda")[0]


def test_softmax_output_is_planned_away():
    def live(pl):
        return [nd.kind for nd in pl.nodes if not nd.attrs.get("dead")]

    lin = NativeGraphEngine.plan_only(_net("linear"), 32)
    assert lin.head_kind == "logits" and live(lin) == ["Conv2D", "MaxPooling2D", "Dense", "Dense"]
    for head in ("softmax", "layer", "activation"):
        pl = NativeGraphEngine.plan_only(_net(head), 32)
        assert pl.head_kind == "probs", head
        assert live(pl) == live(lin), head
        assert pl.head_node.kind == "Dense" and pl.head_node.attrs["logits"], head
        assert pl.head_node.out.shape == (32, 10)
        if head != "softmax":
            sm = pl.nodes[-1]
            assert sm.attrs["dead"] and sm.out.root() is pl.head_node.out, head
            assert pl.describe_plan()["dead"] == lin.describe_plan()["dead"] + 1


def test_r_api_to_categorical_round_trips():
    y = np.array([3, 0, 9, 9, 1])
    oh = r_api.to_categorical(y, 10)
    assert oh.shape == (5, 10) and oh.dtype == np.float32
    assert np.array_equal(oh.argmax(-1), y) and np.array_equal(oh.sum(-1), np.ones(5))
    assert np.array_equal(oh, keras.utils.to_categorical(y, 10))
    assert r_api.to_categorical(y).shape == (5, 10)  # classes from the data
    assert r_api.to_categorical(y, 12.0).shape == (5, 12)  # R passes doubles
