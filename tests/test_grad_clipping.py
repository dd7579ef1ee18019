"""Gradient clipping (clipvalue / clipnorm / global_clipnorm) on the CPU: the optimizer
arguments and their config round trips, the host reference ``clip_grad``, one clipped step
of the generic engine against the closed form (with and without a weight regularizer), and
a world-2 gloo run against world 1."""
import json
import math
import os

import numpy as np
import pytest
import torch

from distributed_amd import keras, launch
from distributed_amd.engine.fused_convnet import FusedConvNetEngine
from distributed_amd.engine.native_graph import NativeGraphEngine
from distributed_amd.ops import reference

L, O, REG = keras.layers, keras.optimizers, keras.regularizers
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "helpers", "clip_worker.py")
MODES = ("clipvalue", "clipnorm", "global_clipnorm")
LR = 0.1


# --- 1. the optimizer arguments ----------------------------------------------------------------
@pytest.mark.parametrize("cls", [O.SGD, O.Adam, O.RMSprop])
def test_constructor_validation(cls):
    for a in MODES:
        for b in MODES:
            if a < b:
                with pytest.raises(ValueError):
                    cls(**{a: 1.0, b: 1.0})
        for bad in (0, 0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                cls(**{a: bad})
        opt = cls(**{a: 0.5})
        assert opt.clipping() == (a, 0.5) and getattr(opt, a) == 0.5
    with pytest.raises(ValueError):
        cls(clipvalue=1.0, clipnorm=1.0, global_clipnorm=1.0)
    assert cls().clipping() == (None, None)
    assert cls(clipnorm=None, clipvalue=2).clipping() == ("clipvalue", 2.0)  # an explicit None is "unset"


@pytest.mark.parametrize("cls", [O.SGD, O.Adam, O.RMSprop])
def test_config_round_trip(cls):
    plain = cls(learning_rate=0.02)
    assert not set(MODES) & set(plain.get_config())  # unset: the config is what it always was
    assert O.get(O.serialize(plain)).clipping() == (None, None)
    for mode in MODES:
        opt = cls(learning_rate=0.02, **{mode: 0.25})
        cfg = opt.get_config()
        assert cfg[mode] == 0.25 and len(set(MODES) & set(cfg)) == 1
        back = O.get(O.serialize(opt))
        assert type(back) is cls and back.clipping() == (mode, 0.25) and back.learning_rate == 0.02
        assert back.get_config() == cfg
    assert O.get({"class_name": "SGD", "config": {"learning_rate": 0.1, "clipnorm": 1.0}}).clipnorm == 1.0
    with pytest.raises(ValueError):
        O.get({"class_name": "SGD", "config": {"clipnorm": 1.0, "clipvalue": 1.0}})


def _dense_model(opt=None, l2=None):
    keras.backend.clear_session()
    kw = dict(kernel_regularizer=REG.l2(l2)) if l2 else {}
    m = keras.Sequential([L.Flatten(input_shape=(4, 4, 1)), L.Dense(8, **kw), L.Dense(3)])
    m.compile(optimizer=opt or O.SGD(LR), loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    return m


@pytest.mark.parametrize("mode", MODES)
def test_save_and_load_model_keep_the_setting(tmp_path, mode):
    m = _dense_model(O.SGD(0.05, momentum=0.9, **{mode: 0.75}))
    path = str(tmp_path / "m.h5")
    m.save(path)
    m2 = keras.models.load_model(path)
    assert type(m2.optimizer) is O.SGD and m2.optimizer.clipping() == (mode, 0.75)
    assert m2.optimizer.get_config() == m.optimizer.get_config()
    plain = _dense_model()
    plain.save(path)
    assert keras.models.load_model(path).optimizer.clipping() == (None, None)


def test_engine_eligibility():
    class _FakeGPUStrategy:
        device = torch.device("cuda")

    def cnn(opt):
        keras.backend.clear_session()
        m = keras.Sequential([L.Conv2D(32, 3, activation="relu", input_shape=(28, 28, 1)), L.MaxPooling2D(),
                              L.Flatten(), L.Dense(64, activation="relu"), L.Dense(10)])
        m.compile(optimizer=opt, loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
        return m

    st = _FakeGPUStrategy()
    assert FusedConvNetEngine.eligible(cnn(O.SGD(0.01)), st) == (True, "")
    for mode in MODES:
        m = cnn(O.SGD(0.01, **{mode: 1.0}))
        assert FusedConvNetEngine.eligible(m, st) == (False, "gradient clipping")
        assert NativeGraphEngine.eligible(m, st) == (True, "")
        m.optimizer.clipnorm = m.optimizer.clipvalue = m.optimizer.global_clipnorm = None
        setattr(m.optimizer, mode, float("nan"))  # set behind the constructor's back
        ok, why = NativeGraphEngine.eligible(m, st)
        assert not ok and mode in why


# --- 2. the host reference ---------------------------------------------------------------------
# three variables of a flat buffer with gaps: norms 5, 0 and 13
TABLE = [(0, 2), (8, 3), (16, 2)]


def _g():
    g = torch.zeros(24)
    g[0:2] = torch.tensor([3.0, -4.0])
    g[16:18] = torch.tensor([-5.0, 12.0])
    g[20] = 7.0  # outside every variable: never touched
    return g


def test_reference_hand_computed():
    g = _g()
    assert reference.clip_grad(g, TABLE, "clipvalue", 4.0) == ([], [])
    np.testing.assert_array_equal(g[[0, 1, 16, 17, 20]].numpy(), [3.0, -4.0, -4.0, 4.0, 7.0])
    assert not g[8:11].any()

    g = _g()
    norms, scales = reference.clip_grad(g, TABLE, "clipnorm", 6.5)
    assert norms == [5.0, 0.0, 13.0]
    assert scales == [1.0, 1.0, 0.5]  # at or below c: exactly 1; the zero gradient: 1, no 0/0
    np.testing.assert_array_equal(g[[0, 1, 16, 17, 20]].numpy(), [3.0, -4.0, -2.5, 6.0, 7.0])
    assert not g[8:11].any() and torch.isfinite(g).all()

    g = _g()
    norms, scales = reference.clip_grad(g, TABLE, "global_clipnorm", 0.5 * math.sqrt(194.0))
    np.testing.assert_allclose(norms, [math.sqrt(194.0)], rtol=1e-15)
    np.testing.assert_allclose(scales, [0.5], rtol=1e-6)
    np.testing.assert_allclose(g[[0, 1, 16, 17]].numpy(), [1.5, -2.0, -2.5, 6.0], rtol=1e-6)
    assert g[20] == 7.0

    g = _g()
    before = g.clone()
    norms, scales = reference.clip_grad(g, TABLE, "global_clipnorm", 100.0)
    assert scales == [1.0] and torch.equal(g, before)  # never clips: the same bits
    g = torch.zeros(24)
    assert reference.clip_grad(g, TABLE, "global_clipnorm", 1.0) == ([0.0], [1.0]) and not g.any()
    with pytest.raises(ValueError):
        reference.clip_grad(_g(), TABLE, "clip", 1.0)


def test_reference_non_finite_norm_poisons_the_update():
    g = _g()
    g[17] = float("inf")
    norms, scales = reference.clip_grad(g, TABLE, "clipnorm", 6.5)
    assert scales[:2] == [1.0, 1.0] and math.isnan(scales[2]) and math.isinf(norms[2])
    assert torch.isnan(g[16:18]).all() and torch.equal(g[0:2], torch.tensor([3.0, -4.0]))
    g = _g()
    g[17] = float("inf")
    norms, scales = reference.clip_grad(g, TABLE, "global_clipnorm", 6.5)
    assert math.isnan(scales[0])
    assert torch.isnan(g[0:2]).all() and torch.isnan(g[8:11]).all() and g[20] == 7.0
    g = _g()
    g[1] = float("nan")
    assert math.isnan(reference.clip_grad(g, TABLE, "clipnorm", 6.5)[1][0])


# --- 3. the generic engine, one step -------------------------------------------------------------
def _init_and_data():
    rng = np.random.default_rng(11)
    w0 = [rng.normal(0, 0.3, (16, 8)).astype(np.float32), rng.normal(0, 0.2, 8).astype(np.float32),
          rng.normal(0, 0.3, (8, 3)).astype(np.float32), np.zeros(3, np.float32)]
    x = rng.random((8, 4, 4, 1)).astype(np.float32)
    y = rng.integers(0, 3, 8)
    return w0, x, y


def _one_step(w0, x, y, l2=None, **clip):
    m = _dense_model(O.SGD(LR, **clip), l2=l2)
    m.set_weights(w0)
    h = m.fit(x, y, batch_size=8, epochs=1, shuffle=False, verbose=0)
    assert m._engine.name == "generic"
    return m.get_weights(), h.history["loss"][0]


def _close(a, b):
    np.testing.assert_allclose(a, np.asarray(b, dtype=np.float32), rtol=1e-5, atol=1e-7)


def test_generic_engine_one_step_closed_forms():
    """Fails without the feature: the arguments were swallowed and every run was the plain one."""
    w0, x, y = _init_and_data()
    w1, loss1 = _one_step(w0, x, y)
    delta = [b.astype(np.float64) - a for a, b in zip(w0, w1)]
    grads = [-d / LR for d in delta]
    gnorm = math.sqrt(sum(float((g * g).sum()) for g in grads))

    wc, lossc = _one_step(w0, x, y, global_clipnorm=0.5 * gnorm)
    assert lossc == loss1  # the reported loss is the unclipped step's
    for a, d, c in zip(w0, delta, wc):
        _close(c, a + 0.5 * d)

    norms = [float(np.sqrt((g * g).sum())) for g in grads]
    c = float(np.median(norms))
    wc, _ = _one_step(w0, x, y, clipnorm=c)
    clipped = [nv > c for nv in norms]
    assert any(clipped) and not all(clipped), norms
    for a, d, b, got, nv, cl in zip(w0, delta, w1, wc, norms, clipped):
        if cl:
            _close(got, a + d * (c / nv))
            assert not np.array_equal(got, b)
        else:
            np.testing.assert_array_equal(got, b)  # scale exactly 1: the plain update's bits

    c = float(np.median(np.abs(np.concatenate([g.ravel() for g in grads]))))
    wc, _ = _one_step(w0, x, y, clipvalue=c)
    for a, g, got in zip(w0, grads, wc):
        assert (np.abs(g) > c).any()
        _close(got, a - LR * np.clip(g, -c, c))

    for mode in MODES:  # c far above every norm / element: bit-identical to the unclipped run
        wc, lossc = _one_step(w0, x, y, **{mode: 1e6})
        assert lossc == loss1
        for b, got in zip(w1, wc):
            np.testing.assert_array_equal(got, b)


def test_regularizer_gradient_is_inside_the_clipped_quantity():
    w0, x, y = _init_and_data()
    l2 = 0.5
    wp, _ = _one_step(w0, x, y)  # the data gradient alone
    grads = [-(b.astype(np.float64) - a) / LR for a, b in zip(w0, wp)]
    grads[0] = grads[0] + 2 * l2 * w0[0].astype(np.float64)  # what the update rule consumes
    norms = [float(np.sqrt((g * g).sum())) for g in grads]
    gnorm = math.sqrt(sum(nv * nv for nv in norms))
    data_norm0 = float(np.sqrt(((grads[0] - 2 * l2 * w0[0]) ** 2).sum()))
    assert norms[0] > 2 * data_norm0  # the penalty dominates the kernel's norm: leaving it out would show

    wc, _ = _one_step(w0, x, y, l2=l2, global_clipnorm=0.5 * gnorm)
    for a, g, got in zip(w0, grads, wc):
        _close(got, a - LR * 0.5 * g)
    c = 0.5 * norms[0]
    assert c > data_norm0  # clipping the data gradient alone would not clip the kernel
    wc, _ = _one_step(w0, x, y, l2=l2, clipnorm=c)
    for a, g, nv, got in zip(w0, grads, norms, wc):
        _close(got, a - LR * g * (c / max(nv, c)))
    c = float(np.median(np.abs(grads[0])))
    wc, _ = _one_step(w0, x, y, l2=l2, clipvalue=c)
    for a, g, got in zip(w0, grads, wc):
        _close(got, a - LR * np.clip(g, -c, c))


# --- 4. world 2 over gloo ------------------------------------------------------------------------
@pytest.mark.dist
@pytest.mark.timeout(300)
def test_world_2_matches_world_1(tmp_path):
    def run(world, per):
        d = tmp_path / f"w{world}"
        d.mkdir()
        env = {"DAMD_DEVICE": "cpu", "DAMD_TEST_OUT": str(d), "PYTHONPATH": ROOT, "OMP_NUM_THREADS": "2",
               "DAMD_LOG_LEVEL": "WARNING", "DAMD_TEST_PER_REPLICA": str(per)}
        res = launch.launch_script([WORKER], nproc=world, env=env, timeout=240)
        assert res.ok, res.returncodes
        out = []
        for r in range(world):
            w = dict(np.load(os.path.join(d, f"rank{r}.npz")))
            with open(os.path.join(d, f"rank{r}.json")) as f:
                out.append((w, json.load(f)))
        return out

    (w0, j0), (w1, j1) = run(2, 4)
    ((ws, js),) = run(1, 8)
    assert j0["world"] == 2 and js["world"] == 1
    assert set(w0) == set(w1) == set(ws) and len(w0) == 16
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k  # replicas stay bitwise mirrored
        # the tolerances of tests/test_regularizers.py's world-2 versus world-1 comparison
        np.testing.assert_allclose(w0[k], ws[k], rtol=1e-4, atol=1e-6, err_msg=k)
    assert j0["runs"] == j1["runs"]
    for mode in MODES:
        assert j0["runs"][mode]["iterations"] == js["runs"][mode]["iterations"] == 2
        np.testing.assert_allclose(j0["runs"][mode]["loss"], js["runs"][mode]["loss"], rtol=1e-5)
        # every mode really clipped: the weights are not where the unclipped run put them
        assert any(not np.array_equal(ws[f"{mode}/{i}"], ws[f"none/{i}"]) for i in range(4)), mode
