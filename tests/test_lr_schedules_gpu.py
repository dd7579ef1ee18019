"""Learning-rate schedules on the GPU: the rate the opt_step kernel evaluates from the
device-side iteration count against the fp64 closed form and the host's integer step logic,
three optimizer steps against ``apply_flat``, per-bucket launches, rejected descriptors, and
whole native-graph runs of the reference MNIST CNN (bitwise against a float rate driven from
the host, graph replay, per-bucket updates, the generic engine)."""
import os

import numpy as np
import pytest
import torch

import distributed_amd as tf
from distributed_amd.engine.ctrl import C_CUR3, C_IT, C_LR
from distributed_amd.ops import hip as H
from distributed_amd.ops import reference as R

import test_regularizers_gpu as TR
from test_native_graph_gpu import _data, _mnist

pytestmark = pytest.mark.gpu
dev = "cuda"
O = tf.keras.optimizers
S = tf.keras.optimizers.schedules

# test_regularizers_gpu's layout and, as in test_grad_clipping_gpu, one variable of several blocks
SIZES = TR.SIZES + (10000,)
COEF = TR.COEF + (None,)


class _Flat(TR._Flat):
    """test_regularizers_gpu's opt_step state with the schedule descriptor."""

    def step(self, t, g, sched=None, splits=None, tab=None):
        self.ctrl[C_CUR3] = t
        G = g.to(dev)
        if sched is not None:
            tab = H.lr_table(sched, dev)
        cuts = [0] + list(splits or []) + [self.n]
        for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            self.C.opt_step(self.P.data_ptr() + 4 * lo, G.data_ptr() + 4 * lo, *(s.data_ptr() + 4 * lo for s in self.S),
                            self.Pb.data_ptr() + 2 * lo, hi - lo, self.ctrl.data_ptr(), self.tail.data_ptr(), self.kind,
                            *map(float, self.args[:5]), self.args[5], torch.cuda.current_stream().cuda_stream,
                            book=int(k == len(cuts) - 2), lr=tab.data_ptr() if tab is not None else 0)
        torch.cuda.synchronize()

    def rate(self):
        return float(self.ctrl[:1].view(torch.float32).item())


def _device_rates(sched, steps):
    """The rate the bookkeeping launch stored in ctrl's lr word for each step (t = step + 1)."""
    f = _Flat(torch.zeros(8), O.SGD(0.5))
    g = torch.zeros(8)
    out = []
    for k in steps:
        f.ctrl[C_LR] = TR._i(-1.0)  # a rate nobody computes: the launch must overwrite it
        f.step(k + 1, g, sched)
        assert int(f.ctrl[C_IT]) == k + 1
        out.append(f.rate())
    return out


# the steps the fp32 mirror's own deviation E was first measured over, and every edge
STEPS = sorted(set(range(41)) | {49, 50, 51, 99, 100, 101, 1000})
ACCURACY = {"exponential": S.ExponentialDecay(0.1, 7, 0.5),
            "inverse_time": S.InverseTimeDecay(0.1, 7, 0.5),
            "polynomial_2": S.PolynomialDecay(0.1, 50, 1e-3, power=2.0),
            "polynomial_half": S.PolynomialDecay(0.1, 50, 1e-3, power=0.5),
            "cosine": S.CosineDecay(0.1, 50, alpha=0.01),
            "cosine_warmup": S.CosineDecay(0.1, 50, alpha=0.01, warmup_target=0.4, warmup_steps=5)}


def _bound(sched, steps):
    """(E, 4 E + 2) in ulps of the initial rate: E = the deviation of the fp32 host mirror from
    the fp64 closed form over ``steps``; 4x for a device powf / cosf allowed 2 ulp against
    numpy's 1 and for fma contraction, + 2 for the final roundings."""
    ulp = float(np.spacing(np.float32(sched.initial_learning_rate)))
    e = max(abs(R.lr_schedule32(sched, k) - sched(k)) for k in steps) / ulp
    return ulp, e, 4.0 * e + 2.0


@pytest.mark.parametrize("name", list(ACCURACY))
def test_rate_accuracy(name):
    sched = ACCURACY[name]
    ds = sched.decay_steps
    steps = sorted(set(STEPS) | {0, 1, ds - 1, ds, ds + 1, 2 * ds} | ({4, 5, 6, 54, 55, 56} if "warmup" in name else set()))
    ulp, e, bound = _bound(sched, steps)
    got = _device_rates(sched, steps)
    dev_ulps = max(abs(a - sched(k)) for a, k in zip(got, steps)) / ulp
    mirror = max(abs(a - R.lr_schedule32(sched, k)) for a, k in zip(got, steps)) / ulp
    print(f"{name}: device vs fp64 {dev_ulps:.2f} ulp of the initial rate (mirror E {e:.2f}, bound {bound:.2f}); "
          f"device vs fp32 mirror {mirror:.2f} ulp")
    assert dev_ulps <= bound


def test_piecewise_values_are_bit_exact():
    bounds = [3, 10, 11, 40, 1000]
    values = [0.4, 0.3, 0.2, 0.1, 0.05, 0.025]
    sched = S.PiecewiseConstantDecay(bounds, values)
    steps = sorted({0, 1, 2000} | set(bounds) | {b + 1 for b in bounds})
    for k, got in zip(steps, _device_rates(sched, steps)):
        assert got == float(np.float32(sched(k))), k
    full = S.PiecewiseConstantDecay(list(range(2, 2 + 2 * H.LR_MAX_BOUNDS, 2)), [0.01 * (i + 1) for i in range(17)])
    steps = list(range(0, 2 * H.LR_MAX_BOUNDS + 5))
    for k, got in zip(steps, _device_rates(full, steps)):
        assert got == float(np.float32(full(k))), k
    assert _device_rates(S.PiecewiseConstantDecay([], [0.125]), [0, 9]) == [0.125, 0.125]


def test_integer_step_logic_matches_the_host():
    # staircase: 1 / (1 + p) names p = step // 7 exactly
    st = S.InverseTimeDecay(1.0, 7, 1.0, staircase=True)
    steps = [0, 1, 6, 7, 8, 13, 14, 15, 699, 700, 701, (1 << 24) + 6, (1 << 24) + 7]
    for k, got in zip(steps, _device_rates(st, steps)):
        # (one division: 2.5 ulp at the most)
        assert round(1.0 / got - 1.0) == k // 7 and abs(got - st(k)) <= 4 * np.spacing(np.float32(got)), k
    se = S.ExponentialDecay(0.5, 7, 0.5, staircase=True)  # one p, one rate, for a whole stair
    steps = [0, 6, 7, 13, 14, 20, 21]
    a = _device_rates(se, steps)
    assert a[0] == a[1] > a[2] == a[3] > a[4] == a[5] > a[6]
    ulp, _, bound = _bound(se, steps)
    assert max(abs(v - se(k)) for v, k in zip(a, steps)) <= bound * ulp
    # cycle: d = 10 ceil(step / 10), max(1, .) at step 0; one step on the wrong side shows as >= 0.05
    cy = S.PolynomialDecay(1.0, 10, 0.0, power=1.0, cycle=True)
    steps = [0, 1, 9, 10, 11, 19, 20, 21, 30, 31, 1000, 1001]
    for k, got in zip(steps, _device_rates(cy, steps)):
        assert abs(got - cy(k)) <= 4 * float(np.spacing(np.float32(1.0))), k
    assert _device_rates(cy, [0, 10, 20])[1:] == [0.0, 0.0]
    # clamps: past decay_steps the rate keeps the bits of step == decay_steps
    for sched in (ACCURACY["polynomial_2"], ACCURACY["polynomial_half"], ACCURACY["cosine"]):
        a = _device_rates(sched, [50, 51, 100, 1000, 1 << 25])
        assert len(set(a)) == 1, a
    assert _device_rates(ACCURACY["polynomial_2"], [50]) == [float(np.float32(1e-3))]
    w = ACCURACY["cosine_warmup"]  # the warm-up branch: linear below step 5, the target at it, clamp at 55
    a = _device_rates(w, [4, 5, 55, 56, 500])
    ulp, _, bound = _bound(w, [4, 5])
    assert abs(a[0] - 0.34) <= bound * ulp and abs(a[1] - 0.4) <= bound * ulp and a[2] == a[3] == a[4]
    z = S.CosineDecay(0.1, 50, warmup_target=0.4, warmup_steps=0)
    assert _device_rates(z, [0]) == [float(np.float32(0.4))]


def test_no_descriptor_leaves_ctrl_lr_alone():
    f = _Flat(torch.ones(8), O.SGD(0.5))
    f.step(1, torch.ones(8))
    assert f.rate() == 0.5 and torch.equal(f.P.cpu(), torch.full((8,), 0.5))
    f.step(2, torch.ones(8), S.PiecewiseConstantDecay([0], [0.5, 0.25]))  # step 1: past the boundary
    assert f.rate() == 0.25 and torch.equal(f.P.cpu(), torch.full((8,), 0.25))


WEIGHT_CASES = {
    "sgd_nesterov": (lambda lr: O.SGD(learning_rate=lr, momentum=0.9, nesterov=True), S.ExponentialDecay(0.05, 2, 0.5)),
    "adam": (lambda lr: O.Adam(learning_rate=lr), S.CosineDecay(1e-3, 4, alpha=0.1)),
    "rmsprop_momentum": (lambda lr: O.RMSprop(learning_rate=lr, momentum=0.9), S.PolynomialDecay(5e-4, 3, 1e-5, power=2.0)),
}


@pytest.mark.parametrize("name", list(WEIGHT_CASES))
def test_opt_step_with_schedule_matches_reference(name):
    """opt_step with the descriptor against the Keras optimizer's own apply_flat on the CPU
    under the same schedule, three steps (test_opt_step_with_table_matches_reference's
    tolerances); several launches with offsets == the single launch, bitwise."""
    make, sched = WEIGHT_CASES[name]
    assert name in TR._opt_cases()
    offs, n, _ = TR._layout(SIZES, COEF)
    p0 = TR._flat(1, offs, n, SIZES)
    opt_h = make(sched)
    opt_h.ensure_slots(n, torch.device("cpu"))
    ph = p0.clone()
    one, two = _Flat(p0, make(0.5)), _Flat(p0, make(0.5))
    for t in range(1, 4):
        g = TR._flat(10 + t, offs, n, SIZES, scale=0.1 if t % 2 else 1.0, zeros=False)
        one.step(t, g, sched)
        two.step(t, g, sched, splits=[offs[2], offs[4], offs[5] + 4096])  # as the clipvalue test splits
        opt_h.apply_flat(ph, g)
        torch.testing.assert_close(one.P.cpu(), ph, rtol=1e-5, atol=1e-6)
        assert int(one.ctrl[C_IT]) == t and int(two.ctrl[C_IT]) == t
        ulp, _, bound = _bound(sched, [t - 1])
        assert one.rate() == two.rate() and abs(one.rate() - sched(t - 1)) <= bound * ulp
        for i, nm in enumerate(one.names):
            if nm:
                torch.testing.assert_close(one.S[i].cpu(), opt_h.slots[nm], rtol=1e-5, atol=1e-7)
        for a, b in zip(one.state(), two.state()):
            assert a.tobytes() == b.tobytes()
    assert torch.equal(one.Pb, one.P.bfloat16())
    assert opt_h.iterations == 3


def test_opt_step_rejects_bad_tables():
    f = _Flat(torch.zeros(8), O.SGD(0.5))
    g = torch.zeros(8)
    good = H.lr_table(S.ExponentialDecay(0.1, 7, 0.5))
    assert good.dtype == torch.int32 and good.numel() == H.LR_WORDS and good.data_ptr() % 16 == 0
    f.step(1, g, tab=good)

    def bad(**words):
        t = good.clone()
        for i, v in words.items():
            t[int(i[1:])] = v
        return t

    piece = H.lr_table(S.PiecewiseConstantDecay([1, 2], [0.1, 0.2, 0.3]))
    over = piece.clone()
    over[7] = H.LR_MAX_BOUNDS + 1
    unsorted = piece.clone()
    unsorted[8], unsorted[9] = 2, 2
    shifted = torch.zeros(H.LR_WORDS + 4, dtype=torch.int32)
    shifted[1:1 + H.LR_WORDS] = good
    cases = {"kind 0": bad(w0=0), "kind 6": bad(w0=6), "kind -1": bad(w0=-1), "decay_steps 0": bad(w2=0),
             "decay_steps -7": bad(w2=-7), "decay_steps 2^24 + 1": bad(w2=(1 << 24) + 1),
             "too many pieces": over, "negative pieces": bad(w0=4, w7=-1), "boundaries not increasing": unsorted,
             "warmup_steps -1": bad(w0=5, w1=1, w3=-1), "misaligned": shifted[1:1 + H.LR_WORDS]}
    before = f.state()
    for what, t in cases.items():
        with pytest.raises(RuntimeError):
            f.step(2, g, tab=t)
        assert int(f.ctrl[C_IT]) == 1, what  # nothing was launched
    for a, b in zip(before, f.state()):
        np.testing.assert_array_equal(a, b)
    for s in (S.ExponentialDecay(0.1, 7.5, 0.5), S.PiecewiseConstantDecay(list(range(17)), [0.1] * 18)):
        with pytest.raises(ValueError):
            H.lr_table(s)


# --- the native engine end to end ---------------------------------------------------------------
def _fit(build, x, y, init, optimizer, epochs=1, steps=None, callbacks=None, graph=True, device=None, native=True,
         **extra):
    """One fit under DAMD_STRICT_NATIVE=1 / DAMD_FUSED=1 (a scheduled model must land on
    native_graph by itself).  Returns (weights, history, engine name, iterations, ctrl's rate)."""
    env = {"DAMD_NATIVE_GRAPH": "1" if native else "0", "DAMD_FUSED": "1", "DAMD_GRAPH": "1" if graph else "0"}
    if native:
        env["DAMD_STRICT_NATIVE"] = "1"
    if device:
        env["DAMD_DEVICE"] = device
    env.update(extra)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    from distributed_amd.parallel import runtime

    try:
        runtime.shutdown()
        tf.keras.backend.clear_session()
        m = build()
        m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=optimizer(),
                  metrics=["accuracy"])
        m.set_weights(init)
        h = m.fit(x, y, batch_size=32, epochs=epochs, steps_per_epoch=steps, shuffle=False, verbose=0,
                  callbacks=callbacks)
        eng = m._engine
        rate = None
        if eng.name == "native_graph":
            torch.cuda.synchronize()
            rate = float(eng.ctrl[:1].view(torch.float32).item())
        return m.get_weights(), h.history, eng.name, int(m.optimizer.iterations), rate
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        runtime.shutdown()


COSINE = S.CosineDecay(0.05, 6, alpha=0.1, warmup_target=0.1, warmup_steps=2)


@pytest.fixture(scope="module")
def mnist_case():
    tf.set_seed(7)
    tf.keras.backend.clear_session()
    init = _mnist().get_weights()
    x, y = _data(96, (28, 28, 1), 10)
    # four CosineDecay steps through the captured graph: the base of the bitwise comparisons
    base = _fit(_mnist, x[:64], y[:64], init, lambda: O.SGD(COSINE, momentum=0.9), epochs=2)
    assert base[2] == "native_graph"
    return init, x, y, base


def _bitwise(a, b):
    for u, v in zip(a[0], b[0]):
        np.testing.assert_array_equal(u, v)
    assert a[1] == b[1] and a[2] == b[2] == "native_graph" and a[3] == b[3]


def test_piecewise_equals_the_float_rate_set_per_epoch(mnist_case):
    """values[0] holds while step <= boundaries[0]: with 2 steps per epoch the boundary 1 puts
    steps 0, 1 on a and steps 2, 3 on b -- the rates LearningRateScheduler sets per epoch."""
    init, x, y, _ = mnist_case
    a, b = 0.05, 0.0125
    sch = _fit(_mnist, x[:64], y[:64], init, lambda: O.SGD(S.PiecewiseConstantDecay([1], [a, b]), momentum=0.9), epochs=2)
    cb = [tf.keras.callbacks.LearningRateScheduler(lambda e: [a, b][e])]
    flt = _fit(_mnist, x[:64], y[:64], init, lambda: O.SGD(a, momentum=0.9), epochs=2, callbacks=cb, DAMD_FUSED="0")
    _bitwise(sch, flt)
    assert sch[3] == 4 and sch[4] == flt[4] == float(np.float32(b))
    one = _fit(_mnist, x[:64], y[:64], init, lambda: O.SGD(a, momentum=0.9), epochs=2, DAMD_FUSED="0")
    assert any(not np.array_equal(u, v) for u, v in zip(one[0], sch[0]))  # b was really used


def test_constant_schedule_is_the_plain_run(mnist_case):
    init, x, y, _ = mnist_case
    sch = _fit(_mnist, x[:64], y[:64], init, lambda: O.SGD(S.ExponentialDecay(0.05, 3, decay_rate=1.0)), epochs=2)
    flt = _fit(_mnist, x[:64], y[:64], init, lambda: O.SGD(0.05), epochs=2, DAMD_FUSED="0")
    _bitwise(sch, flt)


def test_replay_and_buckets_are_bitwise(mnist_case):
    init, x, y, base = mnist_case
    opt = lambda: O.SGD(COSINE, momentum=0.9)  # noqa: E731
    _bitwise(base, _fit(_mnist, x[:64], y[:64], init, opt, epochs=2, graph=False))
    _bitwise(base, _fit(_mnist, x[:64], y[:64], init, opt, epochs=2, DAMD_BUCKET_OPT="1", DAMD_BUCKET_MB="0.05"))


def test_iterations_and_reported_rate(mnist_case):
    *_, base = mnist_case
    assert base[3] == 4
    ulp, e, bound = _bound(COSINE, [3])
    d = abs(base[4] - COSINE(3)) / ulp
    print(f"ctrl rate after 4 steps {base[4]!r}, schedule(3) {COSINE(3)!r}: {d:.2f} ulp (E {e:.2f}, bound {bound:.2f})")
    assert d <= bound


def test_three_steps_track_the_generic_engine(mnist_case):
    init, x, y, _ = mnist_case
    opt = lambda: O.SGD(COSINE, momentum=0.9)  # noqa: E731
    nat = _fit(_mnist, x, y, init, opt, steps=3)
    gen = _fit(_mnist, x, y, init, opt, steps=3, native=False, device="cpu")
    assert nat[2] == "native_graph" and gen[2] == "generic" and nat[3] == gen[3] == 3
    print("3 CosineDecay steps: native", nat[1]["loss"], "generic", gen[1]["loss"])
    np.testing.assert_allclose(nat[1]["loss"], gen[1]["loss"], rtol=1e-2)


def test_assigning_a_rate_later_rebuilds_the_descriptor(mnist_case):
    """float -> schedule -> another schedule -> float on a live model: each epoch runs at the
    rate assigned before it, as the float run that LearningRateScheduler drives does."""
    init, x, y, _ = mnist_case
    a, b, c, d = 0.05, 0.0125, 0.025, 0.00625
    cb = [tf.keras.callbacks.LearningRateScheduler(lambda e: [a, b, c, d][e])]
    flt = _fit(_mnist, x[:64], y[:64], init, lambda: O.SGD(a, momentum=0.9), epochs=4, callbacks=cb, DAMD_FUSED="0")
    env = {"DAMD_NATIVE_GRAPH": "1", "DAMD_FUSED": "0", "DAMD_GRAPH": "1", "DAMD_STRICT_NATIVE": "1"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    from distributed_amd.parallel import runtime

    try:
        runtime.shutdown()
        tf.keras.backend.clear_session()
        m = _mnist()
        m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True), optimizer=O.SGD(a, momentum=0.9),
                  metrics=["accuracy"])
        m.set_weights(init)
        losses, engines = [], []
        # iterations 0, 1 at a; 2, 3 at b; 4, 5 at c; 6, 7 at d
        for rate in (None, S.PiecewiseConstantDecay([1], [a, b]), S.PiecewiseConstantDecay([1, 3], [a, b, c]), d):
            if rate is not None:
                m.optimizer.learning_rate = rate
            h = m.fit(x[:64], y[:64], batch_size=32, epochs=1, shuffle=False, verbose=0)
            losses += h.history["loss"]
            engines.append(m._engine)
            assert m._engine.name == "native_graph"
        assert engines[1] is engines[2]  # schedule -> schedule: the same engine, a new descriptor
        assert int(m.optimizer.iterations) == 8
        got = m.get_weights()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        runtime.shutdown()
    assert losses == flt[1]["loss"]
    for u, v in zip(got, flt[0]):
        np.testing.assert_array_equal(u, v)


def test_assigning_a_schedule_without_a_native_form_selects_an_engine_again(mnist_case):
    class MySchedule(S.LearningRateSchedule):
        def __call__(self, step):
            return 0.05

    init, x, y, _ = mnist_case
    env = {"DAMD_NATIVE_GRAPH": "1", "DAMD_FUSED": "1", "DAMD_GRAPH": "1"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    os.environ.pop("DAMD_STRICT_NATIVE", None)
    from distributed_amd.parallel import runtime

    try:
        runtime.shutdown()
        tf.keras.backend.clear_session()
        m = _mnist()
        m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                  optimizer=O.SGD(S.PiecewiseConstantDecay([100], [0.05, 0.01])), metrics=["accuracy"])
        m.set_weights(init)
        m.fit(x[:64], y[:64], batch_size=32, epochs=1, shuffle=False, verbose=0)
        assert m._engine.name == "native_graph"
        m.optimizer.learning_rate = MySchedule()
        h = m.fit(x[:64], y[:64], batch_size=32, epochs=1, shuffle=False, verbose=0)
        assert m._engine.name == "generic" and int(m.optimizer.iterations) == 4
        assert np.isfinite(h.history["loss"]).all()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        runtime.shutdown()


def test_resnet_with_warmup_cosine_trains_on_native_graph():
    tf.set_seed(3)

    def build():
        return tf.models.resnet18(classes=10, input_shape=(32, 32, 3), widths=(16, 32, 32, 64), blocks=(1, 1, 1, 1),
                                  weight_decay=1e-4)

    tf.keras.backend.clear_session()
    init = build().get_weights()
    x, y = _data(64, (32, 32, 3), 10, seed=2)
    sched = S.CosineDecay(0.1, 1000, warmup_target=0.4, warmup_steps=50)
    w, h, eng, it, rate = _fit(build, x, y, init, lambda: O.SGD(learning_rate=sched, momentum=0.9), epochs=2)
    assert eng == "native_graph" and it == 4 and np.isfinite(h["loss"]).all()
    ulp, _, bound = _bound(sched, [3])
    assert abs(rate - sched(3)) <= bound * ulp  # the linear warm-up, three steps in
