"""Weight regularizers (keras/regularizers.py) on the CPU: the Keras surface and its config
round trips, the generic engine's penalty and gradient against the closed form, the penalty
counted once across replicas, engine planning, and the R mirror."""
import json
import os

import numpy as np
import pytest
import torch

from distributed_amd import keras, launch, r_api
from distributed_amd.engine.fused_convnet import FusedConvNetEngine
from distributed_amd.engine.native_graph import NativeGraphEngine

L, REG = keras.layers, keras.regularizers
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "helpers", "reg_worker.py")


class _FakeGPUStrategy:
    device = torch.device("cuda")


def _closed_form(w, l1, l2):
    w = np.asarray(w, dtype=np.float64)
    return l1 * np.abs(w).sum() + l2 * (w * w).sum()


# --- 1. API and config -----------------------------------------------------------------------
def test_api_get_serialize_and_call():
    assert REG.l2().l2 == 0.01 and REG.l2().l1 == 0.0
    assert REG.l1().l1 == 0.01 and REG.l1().l2 == 0.0
    both = REG.get("l1_l2")
    assert isinstance(both, REG.L1L2) and (both.l1, both.l2) == (0.01, 0.01)
    assert REG.get(None) is None
    inst = REG.L1L2(0.3, 0.7)
    assert REG.get(inst) is inst
    d = REG.get({"class_name": "L1L2", "config": {"l1": 0.25, "l2": 0.5}})
    assert isinstance(d, REG.L1L2) and (d.l1, d.l2) == (0.25, 0.5)
    fn = lambda w: (w ** 4).sum()  # noqa: E731
    assert REG.get(fn) is fn
    cfg = REG.serialize(inst)
    assert cfg == {"class_name": "L1L2", "config": {"l1": 0.3, "l2": 0.7}}
    back = REG.get(json.loads(json.dumps(cfg)))
    assert (back.l1, back.l2) == (0.3, 0.7) and REG.serialize(None) is None
    assert isinstance(inst, REG.Regularizer)
    with pytest.raises(ValueError):
        REG.get("l3")
    w = torch.randn(7, 9, generator=torch.Generator().manual_seed(0))
    w[2, 3] = 0.0
    np.testing.assert_allclose(float(inst(w)), _closed_form(w.numpy(), 0.3, 0.7), rtol=1e-6)


def test_layer_config_round_trip():
    keras.backend.clear_session()
    conv = L.Conv2D(8, 3, kernel_regularizer=REG.l2(1e-4), bias_regularizer="l1", input_shape=(8, 8, 3))
    c = conv.get_config()
    assert c["kernel_regularizer"] == {"class_name": "L1L2", "config": {"l1": 0.0, "l2": 1e-4}}
    assert c["bias_regularizer"] == {"class_name": "L1L2", "config": {"l1": 0.01, "l2": 0.0}}
    conv2 = L.Conv2D.from_config(c)
    assert conv2.kernel_regularizer.l2 == 1e-4 and conv2.bias_regularizer.l1 == 0.01
    dense = L.Dense(4, kernel_regularizer=REG.l1_l2(0.02, 0.05))
    c = dense.get_config()
    assert c["kernel_regularizer"]["config"] == {"l1": 0.02, "l2": 0.05} and c["bias_regularizer"] is None
    d2 = L.Dense.from_config(c)
    assert (d2.kernel_regularizer.l1, d2.kernel_regularizer.l2) == (0.02, 0.05) and d2.bias_regularizer is None
    bn = L.BatchNormalization(gamma_regularizer=REG.l2(0.1), beta_regularizer=REG.l1(0.05))
    c = bn.get_config()
    assert c["gamma_regularizer"]["config"]["l2"] == 0.1 and c["beta_regularizer"]["config"]["l1"] == 0.05
    bn2 = L.BatchNormalization.from_config(c)
    assert bn2.gamma_regularizer.l2 == 0.1 and bn2.beta_regularizer.l1 == 0.05
    # the variables carry them once built
    bn2._maybe_build((None, 4, 4, 8))
    assert bn2.gamma.regularizer is bn2.gamma_regularizer and bn2.moving_mean.regularizer is None
    assert L.Dense(4).get_config()["kernel_regularizer"] is None


def _reg_model():
    keras.backend.clear_session()
    return keras.Sequential([
        L.Conv2D(8, 3, kernel_regularizer=REG.l2(0.05), input_shape=(8, 8, 1)),
        L.BatchNormalization(gamma_regularizer=REG.l2(0.1), beta_regularizer=REG.l1(0.05)),
        L.Flatten(),
        L.Dense(16, activation="relu", kernel_regularizer=REG.l1_l2(0.02, 0.05), bias_regularizer=REG.l1(0.1)),
        L.Dense(3)])


def test_model_save_load_and_losses(tmp_path):
    m = _reg_model()
    m.compile(optimizer="sgd", loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    path = str(tmp_path / "m.h5")
    m.save(path)
    m2 = keras.models.load_model(path)
    names = ("kernel_regularizer", "bias_regularizer", "gamma_regularizer", "beta_regularizer")
    n_reg = 0
    for a, b in zip(m.layers, m2.layers):
        for nm in names:
            ra, rb = getattr(a, nm, None), getattr(b, nm, None)
            assert (ra is None) == (rb is None), (a.name, nm)
            if ra is not None:
                n_reg += 1
                assert (ra.l1, ra.l2) == (rb.l1, rb.l2), (a.name, nm)
    assert n_reg == 5
    # model.losses: one scalar per regularizer, at the current weights
    for mm in (m, m2):
        losses = mm.losses
        assert len(losses) == 5
        want = []
        for l in mm.layers:
            for v in l._weights:
                if v.regularizer is not None:
                    want.append(_closed_form(v.numpy(), v.regularizer.l1, v.regularizer.l2))
        np.testing.assert_allclose([float(t) for t in losses], want, rtol=1e-5)
    # a frozen layer's regularizer still counts
    m.layers[3].trainable = False
    assert len(m.losses) == 5
    # also through model_from_json (functional + sequential share _layer_from_config)
    m3 = keras.models.model_from_json(m.to_json())
    assert m3.layers[3].bias_regularizer.l1 == 0.1


def test_unsupported_regularizer_kwargs_warn():
    with pytest.warns(UserWarning, match="activity_regularizer"):
        L.Dense(4, activity_regularizer=REG.l2())
    with pytest.warns(UserWarning, match="kernel_constraint"):
        L.Conv2D(8, 3, kernel_constraint=lambda w: w)


def test_resnet_weight_decay_argument():
    from distributed_amd.models import resnet18

    keras.backend.clear_session()
    kw = dict(classes=10, input_shape=(32, 32, 3), widths=(16, 32, 32, 64), blocks=(1, 1, 1, 1))
    plain = resnet18(**kw)
    assert plain.losses == [] and not plain._regularized()
    keras.backend.clear_session()
    wd = resnet18(weight_decay=1e-4, **kw)
    regd = wd._regularized()
    kernels = [w for l in wd.layers if isinstance(l, (L.Conv2D, L.Dense)) for w in [l.kernel]]
    assert len(regd) == len(kernels) and {id(v) for v, _ in regd} == {id(k) for k in kernels}
    assert all((r.l1, r.l2) == (0.0, 1e-4) for _, r in regd)


# --- 2. generic engine against the closed form --------------------------------------------------
LR, L1K, L2K, L1B = 0.1, 0.02, 0.05, 0.1


def _dense_model(reg, custom=False):
    keras.backend.clear_session()
    if custom:  # the same penalties as plain callables: torch evaluates and differentiates them
        kw = dict(kernel_regularizer=lambda w: L1K * w.abs().sum() + L2K * (w * w).sum(),
                  bias_regularizer=lambda w: L1B * w.abs().sum())
    else:
        kw = dict(kernel_regularizer=REG.l1_l2(L1K, L2K), bias_regularizer=REG.l1(L1B)) if reg else {}
    m = keras.Sequential([L.Flatten(input_shape=(4, 4, 1)), L.Dense(8, **kw), L.Dense(3)])
    m.compile(optimizer=keras.optimizers.SGD(LR), loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    return m


def _dense_init_and_data():
    rng = np.random.default_rng(3)
    w0 = [rng.normal(0, 0.3, (16, 8)).astype(np.float32), rng.normal(0, 0.2, 8).astype(np.float32),
          rng.normal(0, 0.3, (8, 3)).astype(np.float32), np.zeros(3, np.float32)]
    w0[0][2, 5] = 0.0  # sign(0) = 0: no L1 push at an exactly-zero weight
    x = rng.random((8, 4, 4, 1)).astype(np.float32)
    y = rng.integers(0, 3, 8)
    return w0, x, y


@pytest.mark.parametrize("custom", [False, True], ids=["l1l2", "callable"])
def test_generic_engine_closed_form(custom):
    w0, x, y = _dense_init_and_data()
    R = _closed_form(w0[0], L1K, L2K) + _closed_form(w0[1], L1B, 0.0)
    out = {}
    for reg in (True, False):
        m = _dense_model(reg, custom=custom and reg)
        m.set_weights(w0)
        ev = m.evaluate(x, y, batch_size=8, verbose=0)
        h = m.fit(x, y, batch_size=8, epochs=1, shuffle=False, verbose=0)
        assert m._engine.name == "generic"
        out[reg] = (m.get_weights(), h.history["loss"][0], ev)
    (wr, lr_, er), (wp, lp, ep) = out[True], out[False]
    for i, (l1, l2) in ((0, (L1K, L2K)), (1, (L1B, 0.0))):
        w = w0[i].astype(np.float64)
        want = -LR * (2 * l2 * w + l1 * np.sign(w))
        np.testing.assert_allclose(wr[i].astype(np.float64) - wp[i], want, atol=1e-6, rtol=0)
    assert wr[0][2, 5] == wp[0][2, 5]  # the zero entry: exactly the plain update
    for i in (2, 3):  # the unregularized layer is untouched
        np.testing.assert_array_equal(wr[i], wp[i])
    np.testing.assert_allclose(lr_ - lp, R, rtol=1e-5)
    np.testing.assert_allclose(er - ep, R, rtol=1e-5)


def test_frozen_layer_penalty_counts_without_gradient():
    w0, x, y = _dense_init_and_data()
    R = _closed_form(w0[0], L1K, L2K) + _closed_form(w0[1], L1B, 0.0)
    losses = {}
    for reg in (True, False):
        m = _dense_model(reg)
        m.layers[1].trainable = False
        m.set_weights(w0)
        h = m.fit(x, y, batch_size=8, epochs=1, shuffle=False, verbose=0)
        losses[reg] = h.history["loss"][0]
        np.testing.assert_array_equal(m.layers[1].kernel.numpy(), w0[0])
    np.testing.assert_allclose(losses[True] - losses[False], R, rtol=1e-5)


# --- 3. counted once across replicas ------------------------------------------------------------
@pytest.mark.dist
@pytest.mark.timeout(300)
def test_penalty_counted_once_across_replicas(tmp_path):
    def run(world, per):
        d = tmp_path / f"w{world}"
        d.mkdir()
        env = {"DAMD_DEVICE": "cpu", "DAMD_TEST_OUT": str(d), "PYTHONPATH": ROOT, "OMP_NUM_THREADS": "2",
               "DAMD_LOG_LEVEL": "WARNING", "DAMD_TEST_PER_REPLICA": str(per)}
        res = launch.launch_script([WORKER], nproc=world, env=env, timeout=240)
        assert res.ok, res.returncodes
        out = []
        for r in range(world):
            w = [a for a in np.load(os.path.join(d, f"rank{r}.npz")).values()]
            with open(os.path.join(d, f"rank{r}.json")) as f:
                out.append((w, json.load(f)))
        return out

    (w0, j0), (w1, j1) = run(2, 4)
    ((ws, js),) = run(1, 8)
    assert j0["world"] == 2 and js["world"] == 1 and j0["iterations"] == js["iterations"] == 2
    assert all(np.array_equal(a, b) for a, b in zip(w0, w1)) and j0["history"] == j1["history"]
    # the tolerances of tests/test_distributed_cpu.py's world-2 versus world-1 comparison
    for a, b in zip(w0, ws):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(j0["history"]["loss"], js["history"]["loss"], rtol=1e-5)
    # and the penalty is in there: R(w0) of the first step's loss, once
    assert js["penalty0"] > 0.5
    np.testing.assert_allclose(js["first_step_loss"] - js["first_step_data_loss"], js["penalty0"], rtol=1e-5)
    np.testing.assert_allclose(j0["first_step_loss"], js["first_step_loss"], rtol=1e-5)


# --- 4. planning ------------------------------------------------------------------------------
def _cnn(conv_reg=None, dense_reg=None):
    keras.backend.clear_session()
    m = keras.Sequential([L.Conv2D(32, 3, activation="relu", input_shape=(28, 28, 1), kernel_regularizer=conv_reg),
                          L.MaxPooling2D(), L.Flatten(),
                          L.Dense(64, activation="relu", kernel_regularizer=dense_reg, bias_regularizer=dense_reg),
                          L.Dense(10)])
    m.compile(loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=keras.optimizers.SGD(0.01),
              metrics=["accuracy"])
    return m


def test_engine_planning():
    st = _FakeGPUStrategy()
    plain = _cnn()
    assert FusedConvNetEngine.eligible(plain, st) == (True, "")
    assert NativeGraphEngine.plan_only(plain, 32).describe_plan()["reg_segments"] == 0
    m = _cnn(REG.l2(1e-4), REG.l1_l2(1e-5, 1e-4))
    ok, why = FusedConvNetEngine.eligible(m, st)
    assert not ok and "regulariz" in why
    assert NativeGraphEngine.eligible(m, st) == (True, "")
    assert NativeGraphEngine.plan_only(m, 32).describe_plan()["reg_segments"] == 3
    # an L1L2 with both coefficients zero needs no table row
    assert NativeGraphEngine.plan_only(_cnn(REG.L1L2(), None), 32).describe_plan()["reg_segments"] == 0

    def my_penalty(w):
        return (w ** 4).sum()

    for fn, name in ((lambda w: w.abs().sum(), "<lambda>"), (my_penalty, "my_penalty")):
        ok, why = NativeGraphEngine.eligible(_cnn(fn), st)
        assert not ok and why == f"regularizer {name}"
    from distributed_amd.engine.native_infer import NativeInference

    assert NativeInference.eligible(m, "cuda", evaluate=True) == (True, "")
    ok, why = NativeInference.eligible(_cnn(my_penalty), "cuda", evaluate=True)
    assert not ok and "my_penalty" in why
    assert NativeInference.eligible(_cnn(my_penalty), "cuda") == (True, "")  # predict uses no loss


def test_reference_reg_functions():
    from distributed_amd.ops import reference

    P = torch.tensor([0.5, -2.0, 0.0, 3.0, 0.0, 0.0, 0.0, 0.0, 1.0, -1.0])
    table = [(0, 4, 0.1, 0.0), (8, 2, 0.2, 0.5)]
    g = reference.reg_grad(P, table)
    np.testing.assert_allclose(g.numpy(), [0.1, -0.1, 0.0, 0.1, 0, 0, 0, 0, 1.2, -1.2], rtol=1e-6)
    np.testing.assert_allclose(float(reference.reg_penalty(P, table)), 0.1 * 5.5 + 0.2 * 2 + 0.5 * 2, rtol=1e-6)


# --- 5. R mirror ------------------------------------------------------------------------------
def test_r_verbs():
    keras.backend.clear_session()
    m = r_api.pipe(r_api.keras_model_sequential(),
                   lambda o: r_api.layer_conv_2d(o, filters=8, kernel_size=3, input_shape=r_api.c(8, 8, 1),
                                                 kernel_regularizer=r_api.regularizer_l1(0.5)),
                   r_api.layer_flatten,
                   lambda o: r_api.layer_dense(o, units=4, kernel_regularizer=r_api.regularizer_l2(1e-4),
                                               bias_regularizer=r_api.regularizer_l1_l2(l1=0.1, l2=0.2)))
    conv, _, dense = m.layers
    assert (conv.kernel_regularizer.l1, conv.kernel_regularizer.l2) == (0.5, 0.0)
    assert (dense.kernel_regularizer.l1, dense.kernel_regularizer.l2) == (0.0, 1e-4)
    assert (dense.bias_regularizer.l1, dense.bias_regularizer.l2) == (0.1, 0.2)
    assert dense.kernel.regularizer is dense.kernel_regularizer
    assert r_api.regularizer_l2().l2 == 0.01
    src = open(os.path.join(ROOT, "R", "R", "keras_verbs.R")).read()
    ns = open(os.path.join(ROOT, "R", "NAMESPACE")).read()
    for verb in ("regularizer_l1", "regularizer_l2", "regularizer_l1_l2"):
        assert f"{verb} <- function" in src and f"export({verb})" in ns
