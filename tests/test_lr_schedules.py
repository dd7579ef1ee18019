"""Learning-rate schedules on the CPU: the five ``keras.optimizers.schedules`` classes against
their closed forms, the config / JSON / HDF5 round trips, the generic engine against a
plain-torch loop, resuming, the planners' verdicts, a world-2 gloo run against world 1 and
the R verbs.  Before the feature every one of these failed at ``float(learning_rate)``."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_amd import keras, launch, r_api
import distributed_amd as tf
from distributed_amd.engine.fused_convnet import FusedConvNetEngine
from distributed_amd.engine.native_graph import NativeGraphEngine, schedule_ok
from distributed_amd.ops import hip as H
from distributed_amd.ops import reference

L, O = keras.layers, keras.optimizers
S = keras.optimizers.schedules
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "helpers", "sched_worker.py")


def _ap(v):
    """The same double-precision formula, up to the order of its operations."""
    return pytest.approx(v, rel=1e-14, abs=0.0)


def _edge_steps(ds, extra=()):
    return sorted({0, 1, ds - 1, ds, ds + 1, 2 * ds, *extra})


# --- 1. the closed forms, written out independently ----------------------------------------------
def test_module_is_exposed():
    assert tf.keras.optimizers.schedules is S
    for n in ("LearningRateSchedule", "ExponentialDecay", "InverseTimeDecay", "PolynomialDecay",
              "PiecewiseConstantDecay", "CosineDecay", "serialize", "deserialize"):
        assert hasattr(S, n), n
    for c in (S.ExponentialDecay, S.InverseTimeDecay, S.PolynomialDecay, S.PiecewiseConstantDecay, S.CosineDecay):
        assert issubclass(c, S.LearningRateSchedule)


@pytest.mark.parametrize("staircase", [False, True])
def test_exponential_and_inverse_time(staircase):
    init, ds, rate = 0.1, 7, 0.5
    e = S.ExponentialDecay(init, ds, rate, staircase=staircase)
    v = S.InverseTimeDecay(init, ds, rate, staircase=staircase)
    for k in _edge_steps(ds):
        p = float(k // ds) if staircase else k / ds
        got = e(k)
        assert type(got) is float and got == _ap(init * rate ** p), k
        assert v(k) == _ap(init / (1 + rate * p)), k
    assert e(0) == init and v(0) == init
    if staircase:
        assert e(ds - 1) == init and e(ds) == init * rate and e(2 * ds - 1) == init * rate


@pytest.mark.parametrize("power", [1.0, 2.0, 0.5])
def test_polynomial(power):
    init, ds, end = 0.1, 50, 1e-3
    s = S.PolynomialDecay(init, ds, end, power=power)
    c = S.PolynomialDecay(init, ds, end, power=power, cycle=True)
    for k in _edge_steps(ds, (2 * ds + 1, 3 * ds)):
        assert s(k) == _ap((init - end) * (1 - min(k, ds) / ds) ** power + end), k
        d = ds * max(1, math.ceil(k / ds))
        assert c(k) == _ap((init - end) * (1 - k / d) ** power + end), k
    assert s(0) == c(0) == init  # at step 0 the cycle multiplier is 1
    assert s(ds) == s(2 * ds) == end and c(ds) == end
    assert c(ds + 1) > c(ds)  # a new cycle, over 2 * decay_steps
    assert S.PolynomialDecay(0.1, 10).end_learning_rate == 1e-4 and S.PolynomialDecay(0.1, 10).power == 1.0


def test_piecewise_constant():
    s = S.PiecewiseConstantDecay([3, 10, 11], [0.4, 0.3, 0.2, 0.1])
    want = {0: 0.4, 1: 0.4, 3: 0.4, 4: 0.3, 10: 0.3, 11: 0.2, 12: 0.1, 1000: 0.1}
    for k, v in want.items():
        assert s(k) == v, k
    assert S.PiecewiseConstantDecay([], [0.5])(7) == 0.5


def test_cosine_and_warmup():
    init, ds, alpha = 0.1, 50, 0.01

    def cos(i, k):
        return i * ((1 - alpha) * 0.5 * (1 + math.cos(math.pi * min(k, ds) / ds)) + alpha)

    s = S.CosineDecay(init, ds, alpha=alpha)
    for k in _edge_steps(ds):
        assert s(k) == _ap(cos(init, k)), k
    assert s(0) == init and s(ds) == pytest.approx(init * alpha) and s(2 * ds) == s(ds)
    target, ws = 0.4, 5
    w = S.CosineDecay(init, ds, alpha=alpha, warmup_target=target, warmup_steps=ws)
    for k in _edge_steps(ds, (ws - 1, ws, ws + 1, ws + ds, ws + ds + 1)):
        want = init + (target - init) * k / ws if k < ws else cos(target, k - ws)
        assert w(k) == _ap(want), k
    assert w(0) == init and w(ws) == target
    z = S.CosineDecay(init, ds, warmup_target=target, warmup_steps=0)  # no warm-up step at all
    assert z(0) == target
    d = S.CosineDecay(0.1, 10)
    assert d.alpha == 0.0 and d.warmup_target is None and d.warmup_steps == 0


def test_value_errors():
    for bad in (0, -3, 0.0):
        for make in (lambda d: S.ExponentialDecay(0.1, d, 0.5), lambda d: S.InverseTimeDecay(0.1, d, 0.5),
                     lambda d: S.PolynomialDecay(0.1, d), lambda d: S.CosineDecay(0.1, d)):
            with pytest.raises(ValueError):
                make(bad)
    with pytest.raises(ValueError):
        S.PiecewiseConstantDecay([1, 2], [0.1, 0.2])
    with pytest.raises(ValueError):
        S.PiecewiseConstantDecay([1], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        S.PiecewiseConstantDecay([2, 2], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        S.PiecewiseConstantDecay([3, 1], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError):
        S.deserialize({"class_name": "NoSuchDecay", "config": {}})


def test_fp32_mirror_tracks_the_closed_form():
    """ops/reference.py lr_schedule32 (the device kernel's host mirror): piecewise values are
    the float32 of the value, integer logic is exact, the others stay within 2 ulp of the
    initial rate of the fp64 closed form (measured 0.8 to 1.5)."""
    ulp = float(np.spacing(np.float32(0.1)))
    steps = list(range(41)) + [49, 50, 51, 99, 100, 101, 1000]
    for s in (S.ExponentialDecay(0.1, 7, 0.5), S.InverseTimeDecay(0.1, 7, 0.5),
              S.PolynomialDecay(0.1, 50, 1e-3, power=2.0), S.PolynomialDecay(0.1, 50, 1e-3, power=0.5),
              S.CosineDecay(0.1, 50, alpha=0.01)):
        e = max(abs(reference.lr_schedule32(s, k) - s(k)) for k in steps) / ulp
        assert e <= 2.0, (s, e)
    p = S.PiecewiseConstantDecay([3, 10], [0.4, 0.3, 0.2])
    for k in (0, 3, 4, 10, 11):
        assert reference.lr_schedule32(p, k) == float(np.float32(p(k)))
    st = S.ExponentialDecay(0.5, 7, 0.5, staircase=True)
    assert [reference.lr_schedule32(st, k) for k in (6, 7, 13, 14)] == [0.5, 0.25, 0.25, 0.125]


# --- 2. configs ------------------------------------------------------------------------------------
def _all_schedules():
    return [S.ExponentialDecay(0.1, 7, 0.5, staircase=True), S.InverseTimeDecay(0.1, 7, 0.5),
            S.PolynomialDecay(0.1, 50, 1e-3, power=2.0, cycle=True), S.PiecewiseConstantDecay([3, 10], [0.4, 0.3, 0.2]),
            S.CosineDecay(0.1, 50, alpha=0.01, warmup_target=0.4, warmup_steps=5)]


def _same(a, b):
    assert type(a) is type(b) and a.get_config() == b.get_config()
    for k in (0, 1, 4, 5, 6, 7, 49, 50, 51, 100):
        assert a(k) == b(k)


@pytest.mark.parametrize("sched", _all_schedules(), ids=lambda s: type(s).__name__)
def test_config_round_trips(sched):
    _same(type(sched).from_config(sched.get_config()), sched)
    d = S.serialize(sched)
    assert set(d) == {"class_name", "config"} and d["class_name"] == type(sched).__name__
    _same(S.deserialize(json.loads(json.dumps(d))), sched)
    for cls in (O.SGD, O.Adam, O.RMSprop):
        opt = cls(learning_rate=sched)
        assert opt.learning_rate is sched and opt.lr is sched
        cfg = opt.get_config()
        assert cfg["learning_rate"] == d
        back = O.get(json.loads(json.dumps(O.serialize(opt))))
        assert type(back) is cls and back.get_config() == cfg
        _same(back.learning_rate, sched)
    assert O.SGD(lr=sched).learning_rate is sched


def test_float_rate_config_is_unchanged():
    assert O.SGD(0.02).get_config() == {"name": "SGD", "learning_rate": 0.02, "decay": 0.0, "momentum": 0.0,
                                        "nesterov": False}
    assert json.dumps(O.Adam(0.002).get_config()) == (
        '{"name": "Adam", "learning_rate": 0.002, "decay": 0.0, "beta_1": 0.9, "beta_2": 0.999, '
        '"epsilon": 1e-07, "amsgrad": false}')
    assert json.dumps(O.RMSprop(0.5).get_config()) == (
        '{"name": "RMSprop", "learning_rate": 0.5, "decay": 0.0, "rho": 0.9, "momentum": 0.0, '
        '"epsilon": 1e-07, "centered": false}')
    o = O.SGD(0.02)
    o.learning_rate = 1  # a number still becomes a float
    assert type(o.learning_rate) is float and o.learning_rate == 1.0


def _dense_model(opt):
    keras.backend.clear_session()
    m = keras.Sequential([L.Flatten(input_shape=(4, 4, 1)), L.Dense(8, activation="relu"), L.Dense(3)])
    m.compile(optimizer=opt, loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    return m


@pytest.mark.parametrize("sched", _all_schedules(), ids=lambda s: type(s).__name__)
def test_json_and_hdf5_round_trips(tmp_path, sched):
    m = _dense_model(O.SGD(sched, momentum=0.9))
    m2 = keras.models.model_from_json(m.to_json())
    assert [type(l) for l in m2.layers] == [type(l) for l in m.layers]
    path = str(tmp_path / "m.h5")
    m.save(path)
    m3 = keras.models.load_model(path)
    assert type(m3.optimizer) is O.SGD and m3.optimizer.momentum == 0.9
    _same(m3.optimizer.learning_rate, sched)
    assert m3.optimizer.get_config() == m.optimizer.get_config()


# --- 3. the generic engine -------------------------------------------------------------------------
def _data(n, seed=11):
    rng = np.random.default_rng(seed)
    w0 = [rng.normal(0, 0.3, (16, 8)).astype(np.float32), rng.normal(0, 0.2, 8).astype(np.float32),
          rng.normal(0, 0.3, (8, 3)).astype(np.float32), np.zeros(3, np.float32)]
    return w0, rng.random((n, 4, 4, 1)).astype(np.float32), rng.integers(0, 3, n)


def _torch_grads(ws, xb, yb):
    k1, b1, k2, b2 = ws
    h = torch.relu(torch.as_tensor(xb).reshape(len(xb), -1) @ k1 + b1)
    return torch.autograd.grad(F.cross_entropy(h @ k2 + b2, torch.as_tensor(yb).long()), ws)


def _close(got, ws):
    # the tolerances of test_depthwise_api.py::test_generic_training_matches_plain_torch_sgd
    for a, b in zip(got, ws):
        np.testing.assert_allclose(a, b.detach().numpy(), rtol=1e-5, atol=1e-6)


def test_generic_sgd_matches_plain_torch():
    steps, bs = 5, 8
    sched = S.ExponentialDecay(0.2, 2, 0.5)
    w0, x, y = _data(bs * steps)
    m = _dense_model(O.SGD(sched))
    m.set_weights(w0)
    m.fit(x, y, batch_size=bs, epochs=1, shuffle=False, verbose=0)
    assert m._engine.name == "generic" and m.optimizer.iterations == steps
    ws = [torch.tensor(w, requires_grad=True) for w in w0]
    for k in range(steps):
        grads = _torch_grads(ws, x[k * bs:(k + 1) * bs], y[k * bs:(k + 1) * bs])
        with torch.no_grad():
            for w, g in zip(ws, grads):
                w -= sched(k) * g  # the first update uses schedule(0)
    _close(m.get_weights(), ws)
    # the schedule mattered: a constant initial rate ends elsewhere
    c = _dense_model(O.SGD(0.2))
    c.set_weights(w0)
    c.fit(x, y, batch_size=bs, epochs=1, shuffle=False, verbose=0)
    assert np.abs(c.get_weights()[0] - m.get_weights()[0]).max() > 1e-3


def test_generic_adam_matches_plain_torch():
    steps, bs = 3, 8
    sched = S.CosineDecay(0.01, 4, alpha=0.1)
    b1, b2, eps = 0.9, 0.999, 1e-7
    w0, x, y = _data(bs * steps)
    m = _dense_model(O.Adam(sched))
    m.set_weights(w0)
    m.fit(x, y, batch_size=bs, epochs=1, shuffle=False, verbose=0)
    assert m._engine.name == "generic"
    ws = [torch.tensor(w, requires_grad=True) for w in w0]
    ms, vs = [torch.zeros_like(w) for w in ws], [torch.zeros_like(w) for w in ws]
    for k in range(steps):
        grads = _torch_grads(ws, x[k * bs:(k + 1) * bs], y[k * bs:(k + 1) * bs])
        t = k + 1
        lr_t = sched(k) * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        with torch.no_grad():
            for w, g, mm, vv in zip(ws, grads, ms, vs):
                mm.mul_(b1).add_(g, alpha=1 - b1)
                vv.mul_(b2).addcmul_(g, g, value=1 - b2)
                w -= lr_t * mm / (vv.sqrt() + eps)
    _close(m.get_weights(), ws)


@pytest.mark.parametrize("make", [lambda lr: O.SGD(lr, momentum=0.9), lambda lr: O.Adam(lr), lambda lr: O.RMSprop(lr)],
                         ids=["sgd", "adam", "rmsprop"])
def test_constant_schedule_is_the_float_run_bit_for_bit(make):
    w0, x, y = _data(24)
    out = []
    for lr in (0.05, S.ExponentialDecay(0.05, 3, decay_rate=1.0)):
        m = _dense_model(make(lr))
        m.set_weights(w0)
        h = m.fit(x, y, batch_size=8, epochs=1, shuffle=False, verbose=0)
        out.append((m.get_weights(), h.history["loss"]))
    assert out[0][1] == out[1][1]
    for a, b in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(a, b)


def test_user_subclass_trains_on_the_generic_engine():
    class Halving(S.LearningRateSchedule):
        def __call__(self, step):
            return 0.1 / 2 ** step

        def get_config(self):
            return {}

    w0, x, y = _data(16)
    m = _dense_model(O.SGD(Halving()))
    m.set_weights(w0)
    m.fit(x, y, batch_size=8, epochs=1, shuffle=False, verbose=0)
    ws = [torch.tensor(w, requires_grad=True) for w in w0]
    for k in range(2):
        grads = _torch_grads(ws, x[k * 8:(k + 1) * 8], y[k * 8:(k + 1) * 8])
        with torch.no_grad():
            for w, g in zip(ws, grads):
                w -= 0.1 / 2 ** k * g
    _close(m.get_weights(), ws)


def test_resumed_run_continues_the_schedule(tmp_path):
    w0, x, y = _data(24)
    sched = S.PolynomialDecay(0.2, 8, 0.01, power=2.0)

    def fresh():
        m = _dense_model(O.SGD(sched, momentum=0.9))
        m.set_weights(w0)
        return m

    whole = fresh()
    whole.fit(x, y, batch_size=8, epochs=3, shuffle=False, verbose=0)
    part = fresh()
    part.fit(x, y, batch_size=8, epochs=2, shuffle=False, verbose=0)
    path = str(tmp_path / "part.h5")
    part.save(path)
    back = keras.models.load_model(path)
    assert back.optimizer.iterations == 6
    back.fit(x, y, batch_size=8, epochs=1, shuffle=False, verbose=0)
    assert back.optimizer.iterations == whole.optimizer.iterations == 9
    for a, b in zip(back.get_weights(), whole.get_weights()):
        np.testing.assert_array_equal(a, b)


def test_learning_rate_scheduler_callback_refuses_a_schedule():
    w0, x, y = _data(8)
    m = _dense_model(O.SGD(S.CosineDecay(0.1, 10)))
    with pytest.raises(TypeError, match="CosineDecay"):
        m.fit(x, y, batch_size=8, epochs=1, verbose=0, callbacks=[keras.callbacks.LearningRateScheduler(lambda e: 0.1)])
    m = _dense_model(O.SGD(0.1))  # a float rate is set per epoch as ever
    m.fit(x, y, batch_size=8, epochs=2, verbose=0, callbacks=[keras.callbacks.LearningRateScheduler(lambda e: 0.1 / (e + 1))])
    assert m.optimizer.learning_rate == 0.05


# --- 4. the planners ---------------------------------------------------------------------------------
class _FakeGPUStrategy:
    device = torch.device("cuda")


def _cnn(opt):
    keras.backend.clear_session()
    m = keras.Sequential([L.Conv2D(32, 3, activation="relu", input_shape=(28, 28, 1)), L.MaxPooling2D(),
                          L.Flatten(), L.Dense(64, activation="relu"), L.Dense(10)])
    m.compile(optimizer=opt, loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    return m


def test_engine_eligibility():
    st = _FakeGPUStrategy()
    assert FusedConvNetEngine.eligible(_cnn(O.SGD(0.01)), st) == (True, "")
    assert schedule_ok(_cnn(O.SGD(0.01))) == (True, "")
    for sched in _all_schedules() + [S.CosineDecay(0.1, 2 ** 24), S.ExponentialDecay(0.1, 1, 0.5)]:
        for cls in (O.SGD, O.Adam, O.RMSprop):
            m = _cnn(cls(sched))
            assert FusedConvNetEngine.eligible(m, st) == (False, "learning-rate schedule")
            assert NativeGraphEngine.eligible(m, st) == (True, ""), sched
            assert schedule_ok(m) == (True, "")

    class MySchedule(S.LearningRateSchedule):
        def __call__(self, step):
            return 0.1

    class CosineDecay(S.CosineDecay):  # a subclass may compute anything
        pass

    many = S.PiecewiseConstantDecay(list(range(1, 41)), [0.1] * 41)
    assert H.LR_MAX_BOUNDS == 16
    rejected = [(MySchedule(), "learning-rate schedule MySchedule"),
                (CosineDecay(0.1, 10), "learning-rate schedule CosineDecay"),
                (many, "learning-rate schedule: 40 boundaries exceed the table cap 16"),
                (S.ExponentialDecay(0.1, 7.5, 0.5), "decay_steps"),
                (S.CosineDecay(0.1, 2 ** 24 + 1), "decay_steps"),
                (S.CosineDecay(0.1, 10, warmup_target=0.2, warmup_steps=2.5), "warmup_steps"),
                (S.PiecewiseConstantDecay([2.5], [0.1, 0.2]), "boundaries"),
                (S.ExponentialDecay(float("inf"), 7, 0.5), "finite"),
                (S.PolynomialDecay(0.1, 7, power=float("nan")), "finite"),
                (S.PiecewiseConstantDecay([2], [0.1, float("nan")]), "finite")]
    for sched, why in rejected:
        m = _cnn(O.SGD(sched))
        ok, got = NativeGraphEngine.eligible(m, st)
        assert not ok and why in got and got.startswith("learning-rate schedule"), (got, why)
        assert schedule_ok(m) == (ok, got)
    assert NativeGraphEngine.eligible(_cnn(O.SGD(MySchedule())), st)[1] == "learning-rate schedule MySchedule"
    assert NativeGraphEngine.eligible(_cnn(O.SGD(S.PiecewiseConstantDecay(list(range(16)), [0.1] * 17))), st)[0]


# --- 5. world 2 over gloo ----------------------------------------------------------------------------
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
    assert set(w0) == set(w1) == set(ws) and len(w0) == 4 * len(js["runs"])
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k  # replicas stay bitwise mirrored
        # the tolerances of tests/test_grad_clipping.py's world-2 versus world-1 comparison
        np.testing.assert_allclose(w0[k], ws[k], rtol=1e-4, atol=1e-6, err_msg=k)
    assert j0["runs"] == j1["runs"]
    for name in js["runs"]:
        assert j0["runs"][name]["iterations"] == js["runs"][name]["iterations"] == 3
        np.testing.assert_allclose(j0["runs"][name]["loss"], js["runs"][name]["loss"], rtol=1e-5)
        if name != "none":  # every schedule really moved the rate off the constant run's
            assert any(not np.array_equal(ws[f"{name}/{i}"], ws[f"none/{i}"]) for i in range(4)), name


# --- 6. the R verbs ----------------------------------------------------------------------------------
def test_r_verbs():
    e = r_api.learning_rate_schedule_exponential_decay(0.1, 7.0, 0.5, staircase=True)
    assert type(e) is S.ExponentialDecay and e.decay_steps == 7 and type(e.decay_steps) is int and e.staircase
    i = r_api.learning_rate_schedule_inverse_time_decay(0.1, 7.0, 0.5)
    assert type(i) is S.InverseTimeDecay and type(i.decay_steps) is int and not i.staircase
    p = r_api.learning_rate_schedule_polynomial_decay(0.1, 50.0, end_learning_rate=1e-3, power=2.0, cycle=True)
    assert type(p) is S.PolynomialDecay and type(p.decay_steps) is int and p.power == 2.0 and p.cycle
    w = r_api.learning_rate_schedule_piecewise_constant_decay(r_api.c(3.0, 10.0), r_api.c(0.4, 0.3, 0.2))
    assert type(w) is S.PiecewiseConstantDecay and w.boundaries == [3, 10]
    assert all(type(b) is int for b in w.boundaries) and w(4) == 0.3
    c = r_api.learning_rate_schedule_cosine_decay(0.1, 1000.0, warmup_target=0.4, warmup_steps=50.0)
    assert type(c) is S.CosineDecay and type(c.decay_steps) is int and type(c.warmup_steps) is int
    assert c.warmup_steps == 50 and c.warmup_target == 0.4
    for s in (e, i, p, w, c):
        assert H.lr_schedule_ok(s) == (True, "")
    ns = open(os.path.join(ROOT, "R", "NAMESPACE")).read()
    verbs = open(os.path.join(ROOT, "R", "R", "keras_verbs.R")).read()
    for verb in ("learning_rate_schedule_exponential_decay", "learning_rate_schedule_inverse_time_decay",
                 "learning_rate_schedule_polynomial_decay", "learning_rate_schedule_piecewise_constant_decay",
                 "learning_rate_schedule_cosine_decay"):
        assert f"export({verb})" in ns, verb
        assert f"{verb} <- function(" in verbs and f".r()${verb}(" in verbs, verb
