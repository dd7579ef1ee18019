"""Sample and class weights through the native engines end to end: the MNIST CNN (96
samples, batch 32) under DAMD_STRICT_NATIVE=1 -- engine routing, the weighted step of the
native graph engine against its own unweighted step, against the generic engine on the CPU
and against graph replay, and weighted ``evaluate`` through the native inference plan."""
import os

import numpy as np
import pytest

import distributed_amd as tf
from distributed_amd.engine.native_infer import NativeInference
from distributed_amd.keras.utils import to_categorical

from test_native_graph_gpu import _data, _mnist

pytestmark = pytest.mark.gpu

SCE, CCE = tf.keras.losses.SparseCategoricalCrossentropy, tf.keras.losses.CategoricalCrossentropy
N, BATCH = 96, 32


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


def _fit(x, y, init, native=True, loss=SCE, lr=0.05, momentum=0.0, epochs=1, steps=None, shuffle=False, keep=False,
         env=None, **fit_kw):
    """(weights, history, engine name, model) of one short run from ``init``; ``fit_kw``:
    sample_weight / class_weight / validation_data.  ``keep``: the runtime stays up, so the
    model can go on to evaluate."""
    from distributed_amd.parallel import runtime

    if native:
        e = {"DAMD_NATIVE_GRAPH": "1", "DAMD_FUSED": "0", "DAMD_STRICT_NATIVE": "1"}
    else:  # the generic engine in fp32 on the CPU
        e = {"DAMD_NATIVE_GRAPH": "0", "DAMD_FUSED": "0", "DAMD_DEVICE": "cpu"}
    e.update(env or {})
    with _Env(**e):
        runtime.shutdown()
        try:
            tf.keras.backend.clear_session()
            tf.set_seed(3)  # the same epoch permutations in every run
            m = _mnist()
            m.compile(loss=loss(from_logits=True), optimizer=tf.keras.optimizers.SGD(learning_rate=lr,
                                                                                     momentum=momentum),
                      metrics=["accuracy"])
            m.set_weights(init)
            h = m.fit(x, y, batch_size=BATCH, epochs=epochs, steps_per_epoch=steps, shuffle=shuffle, verbose=0,
                      **fit_kw)
            return m.get_weights(), h.history, m._engine.name, m
        finally:
            if not keep:
                runtime.shutdown()


def _init():
    tf.keras.backend.clear_session()
    return _mnist().get_weights()


def _weights(n, seed):
    return np.random.default_rng(seed).uniform(0.0, 3.0, n).astype(np.float32)


def test_engine_routing():
    """A weighted fit of the reference CNN leaves the fused engine for the native graph engine
    (default flags, strict native: no fallback); the next unweighted fit is back on it."""
    from distributed_amd.parallel import runtime

    x, y = _data(N, (28, 28, 1), 10, seed=31)
    with _Env(DAMD_STRICT_NATIVE="1", DAMD_FUSED="1", DAMD_NATIVE_GRAPH="1"):
        runtime.shutdown()
        try:
            tf.keras.backend.clear_session()
            m = _mnist()
            m.compile(loss=SCE(from_logits=True), optimizer=tf.keras.optimizers.SGD(learning_rate=0.05),
                      metrics=["accuracy"])
            h = m.fit(x, y, batch_size=BATCH, epochs=1, verbose=0, sample_weight=_weights(N, 1))
            assert m._engine.name == "native_graph" and np.isfinite(h.history["loss"][0])
            m.fit(x, y, batch_size=BATCH, epochs=1, verbose=0, class_weight={c: 1.0 + c for c in range(10)})
            assert m._engine.name == "native_graph"
            h = m.fit(x, y, batch_size=BATCH, epochs=1, verbose=0)
            assert m._engine.name == "fused_convnet" and np.isfinite(h.history["loss"][0])
        finally:
            runtime.shutdown()


def test_all_ones_weights_are_the_unweighted_step_bitwise():
    x, y = _data(N, (28, 28, 1), 10, seed=32)
    init = _init()
    wu, hu, eu, _ = _fit(x, y, init, momentum=0.9, epochs=2, shuffle=True)
    w1, h1, e1, _ = _fit(x, y, init, momentum=0.9, epochs=2, shuffle=True, sample_weight=np.ones(N, np.float32))
    assert eu == e1 == "native_graph"
    for a, b in zip(wu, w1):
        np.testing.assert_array_equal(a, b)
    assert hu == h1


def test_constant_weight_two_doubles_the_step():
    """A power-of-two scale commutes with every rounding on the path: one SGD step with every
    weight 2.0 moves the weights twice as far, and reports twice the loss."""
    x, y = _data(BATCH, (28, 28, 1), 10, seed=33)
    init = _init()
    wu, hu, _, _ = _fit(x, y, init)
    w2, h2, e2, _ = _fit(x, y, init, sample_weight=np.full(BATCH, 2.0, np.float32))
    assert e2 == "native_graph"
    moved = 0
    for a, u, d in zip(init, wu, w2):
        np.testing.assert_allclose(d - a, 2.0 * (u - a), rtol=0, atol=1e-6)
        moved += int(np.abs(u - a).max() > 1e-5)
    assert moved >= 3  # (the kernels' steps are far above the bound: 2x is not 1x)
    np.testing.assert_allclose(h2["loss"], 2.0 * np.asarray(hu["loss"]), rtol=1e-6)
    assert h2["accuracy"] == hu["accuracy"]


def test_zero_weight_rows_do_not_influence_the_update():
    """A third of the rows get weight 0 and other images: over two shuffled epochs the final
    weights are bit-identical to those from the original images (every contribution of those
    rows is +-0 in a fixed-order sum) -- which they are only if the weights follow the epoch
    permutation on the device."""
    x, y = _data(N, (28, 28, 1), 10, seed=34)
    w = _weights(N, 2) + 0.25
    zero = np.arange(N) % 3 == 1
    w[zero] = 0.0
    x2 = x.copy()
    x2[zero] = _data(N, (28, 28, 1), 10, seed=35)[0][zero]
    init = _init()
    wa, ha, ea, _ = _fit(x, y, init, momentum=0.9, epochs=2, shuffle=True, sample_weight=w)
    wb, hb, eb, _ = _fit(x2, y, init, momentum=0.9, epochs=2, shuffle=True, sample_weight=w)
    assert ea == eb == "native_graph"
    for a, b in zip(wa, wb):
        np.testing.assert_array_equal(a, b)
    assert ha["loss"] == hb["loss"]
    # the rows do count when their weight is not 0: the check above can fail
    wc, _, _, _ = _fit(x2, y, init, momentum=0.9, epochs=2, shuffle=True, sample_weight=w + zero)
    assert not np.array_equal(wa[0], wc[0])


@pytest.mark.parametrize("n", [N, 80])
def test_random_weights_track_the_generic_engine(n):
    """Three steps (n = 80: the last batch has 16 of 32 rows) with weights in [0, 3]."""
    x, y = _data(n, (28, 28, 1), 10, seed=36)
    w = _weights(n, 3)
    init = _init()
    wn, hn, en, _ = _fit(x, y, init, sample_weight=w)
    wr, hr, er, _ = _fit(x, y, init, native=False, sample_weight=w)
    assert en == "native_graph" and er == "generic"
    np.testing.assert_allclose(hn["loss"], hr["loss"], rtol=1e-2)
    _, hp, _, _ = _fit(x, y, init, native=False)
    assert abs(hp["loss"][0] - hr["loss"][0]) > 5e-2 * hr["loss"][0]  # the weights matter at this bound


def test_one_hot_targets_with_class_weight_equal_the_sparse_loss():
    x, y = _data(N, (28, 28, 1), 10, seed=37)
    cw = {c: 0.25 + 0.3 * c for c in range(10)}
    init = _init()
    wd, hd, ed, _ = _fit(x, to_categorical(y, 10), init, loss=CCE, class_weight=cw)
    ws, hs, es, _ = _fit(x, y, init, class_weight=cw)
    assert ed == es == "native_graph"
    for a, b in zip(wd, ws):
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(hd["loss"], hs["loss"], rtol=1e-5)
    assert hd["accuracy"] == hs["accuracy"]


def test_graph_replay_equals_eager():
    x, y = _data(128, (28, 28, 1), 10, seed=38)
    w = _weights(128, 4)
    init = _init()
    wg, hg, eg, _ = _fit(x, y, init, momentum=0.9, steps=4, sample_weight=w, env={"DAMD_GRAPH": "1"})
    we, he, _, _ = _fit(x, y, init, momentum=0.9, steps=4, sample_weight=w, env={"DAMD_GRAPH": "0"})
    assert eg == "native_graph"
    for a, b in zip(wg, we):
        np.testing.assert_array_equal(a, b)
    assert hg == he


def test_weighted_evaluate_and_validation_data():
    """evaluate(sample_weight=) through the native inference plan against the PyTorch loop
    (the bounds of test_loss_heads_train_gpu.py::test_predict_and_evaluate); a second, longer
    call re-stages the grown buffers; fit(validation_data=(x, y, w)) reports that evaluate."""
    from distributed_amd.parallel import runtime

    x, y = _data(1000, (28, 28, 1), 10, seed=39)
    w = _weights(1000, 5)
    try:
        _, _, en, m = _fit(x[:N], y[:N], _init(), momentum=0.9, sample_weight=w[:N], keep=True)
        assert en == "native_graph"
        for n in (600, 1000):  # 128-row batches: both end in a short batch
            fn = lambda: m.evaluate(x[:n], y[:n], batch_size=128, verbose=0, return_dict=True,  # noqa: E731
                                    sample_weight=w[:n])
            with _Env(DAMD_NATIVE_INFER="0"):
                ref = fn()
            with _Env(DAMD_NATIVE_INFER="1", DAMD_STRICT_NATIVE="1"):
                nat = fn()
                plain = m.evaluate(x[:n], y[:n], batch_size=128, verbose=0, return_dict=True)
            assert any(isinstance(p, NativeInference) for p in m._infer_plans.values())
            assert abs(nat["loss"] - ref["loss"]) < 1e-2 * ref["loss"]
            assert abs(nat["accuracy"] - ref["accuracy"]) <= 5 / 1000
            assert nat["accuracy"] == plain["accuracy"]  # unweighted
            assert abs(nat["loss"] - plain["loss"]) > 5e-2 * plain["loss"]  # (mean weight 1.5)
        with _Env(DAMD_NATIVE_INFER="1", DAMD_STRICT_NATIVE="1", DAMD_FUSED="0"):
            h = m.fit(x[:N], y[:N], batch_size=BATCH, epochs=1, shuffle=False, verbose=0, sample_weight=w[:N],
                      validation_data=(x[N:300], y[N:300], w[N:300]))
            ev = m.evaluate(x[N:300], y[N:300], batch_size=BATCH, verbose=0, return_dict=True,
                            sample_weight=w[N:300])
        assert h.history["val_loss"][0] == ev["loss"] and h.history["val_accuracy"][0] == ev["accuracy"]
    finally:
        runtime.shutdown()
