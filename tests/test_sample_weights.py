"""Sample and class weights in ``fit`` / ``evaluate`` on the CPU (the generic engine): one
weighted SGD step against the closed form, the argument forms and their validation, the
validation split / data, the R mirror, engine routing, and a world-2 gloo run against
world 1.  Keras SUM_OVER_BATCH_SIZE: loss = sum w_i l_i / N, gradient = sum w_i grad l_i / N,
N the number of rows (not the sum of the weights); metrics stay unweighted."""
import json
import os

import numpy as np
import pytest
import torch

from distributed_amd import keras, launch, r_api
from distributed_amd.engine.fused_convnet import FusedConvNetEngine
from distributed_amd.engine.native_graph import NativeGraphEngine
from distributed_amd.keras.utils import resolve_sample_weights, to_categorical

L, O = keras.layers, keras.optimizers
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "helpers", "weights_worker.py")
LR = 0.1
CW = {0: 1.0, 1: 2.5, 2: 0.5}


def _model(one_hot=False):
    keras.backend.clear_session()
    m = keras.Sequential([L.Flatten(input_shape=(4, 4, 1)), L.Dense(8), L.Dense(3)])
    loss = (keras.losses.CategoricalCrossentropy if one_hot else keras.losses.SparseCategoricalCrossentropy)
    m.compile(optimizer=O.SGD(LR), loss=loss(from_logits=True), metrics=["accuracy"])
    return m


def _init_and_data(n=16, seed=11):
    rng = np.random.default_rng(seed)
    w0 = [rng.normal(0, 0.3, (16, 8)).astype(np.float32), rng.normal(0, 0.2, 8).astype(np.float32),
          rng.normal(0, 0.3, (8, 3)).astype(np.float32), np.zeros(3, np.float32)]
    x = rng.random((n, 4, 4, 1)).astype(np.float32)
    y = rng.integers(0, 3, n)
    sw = (0.25 + 0.2 * np.arange(n)).astype(np.float32)  # distinct
    sw[2], sw[5] = 0.0, 3.5
    return w0, x, y, sw


def _fit(w0, x, y, batch=None, one_hot=False, epochs=1, **kw):
    m = _model(one_hot)
    m.set_weights(w0)
    h = m.fit(x, y, batch_size=batch or len(x), epochs=epochs, shuffle=False, verbose=0, **kw)
    assert m._engine.name == "generic"
    return m, m.get_weights(), h.history


def _host(w0, x, y, sw):
    """fp64 autograd: (per-sample losses, gradients of sum w l / N, per-sample correct)."""
    ws = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in w0]
    xt = torch.tensor(x.reshape(len(x), -1), dtype=torch.float64)
    z = (xt @ ws[0] + ws[1]) @ ws[2] + ws[3]
    ls = torch.nn.functional.cross_entropy(z, torch.tensor(y, dtype=torch.long), reduction="none")
    total = (ls * torch.tensor(sw, dtype=torch.float64)).sum() / len(x)
    grads = torch.autograd.grad(total, ws)
    corr = (z.argmax(-1) == torch.tensor(y)).double()
    return ls.detach().numpy(), [g.numpy() for g in grads], corr.numpy()


def test_one_weighted_sgd_step_closed_form():
    """Fails without the feature: ``fit`` raised NotImplementedError for either argument."""
    w0, x, y, sw = _init_and_data()
    assert len(set(sw.tolist())) == len(sw) and 0.0 in sw and 3.5 in sw
    _, w1, h = _fit(w0, x, y, sample_weight=sw)
    ls, grads, corr = _host(w0, x, y, sw)
    for a, g, got in zip(w0, grads, w1):
        np.testing.assert_allclose(got, (a - LR * g).astype(np.float32), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(h["loss"][0], float((ls * sw).sum() / len(x)), rtol=1e-6)
    _, wp, hp = _fit(w0, x, y)
    assert h["accuracy"] == hp["accuracy"] and h["accuracy"][0] == pytest.approx(corr.mean())  # unweighted
    assert not np.array_equal(wp[0], w1[0])
    # the divisor is the number of rows, not the sum of the weights
    np.testing.assert_allclose(hp["loss"][0], float(ls.mean()), rtol=1e-6)


def test_all_ones_weights_are_the_unweighted_run_bitwise():
    w0, x, y, _ = _init_and_data()
    _, wp, hp = _fit(w0, x, y, batch=8, epochs=2)
    for kw in (dict(sample_weight=np.ones(16, np.float32)), dict(sample_weight=np.ones((16, 1))),
               dict(class_weight={0: 1, 1: 1, 2: 1})):
        _, w1, h1 = _fit(w0, x, y, batch=8, epochs=2, **kw)
        assert h1 == hp
        for a, b in zip(wp, w1):
            np.testing.assert_array_equal(a, b)


def test_class_weight_forms():
    w0, x, y, sw = _init_and_data()
    eq = np.array([CW[int(c)] for c in y], dtype=np.float32)
    _, wa, ha = _fit(w0, x, y, class_weight=CW)
    _, wb, hb = _fit(w0, x, y, sample_weight=eq)
    assert ha == hb and not np.array_equal(wa[0], _fit(w0, x, y)[1][0])
    for a, b in zip(wa, wb):
        np.testing.assert_array_equal(a, b)
    # one-hot targets: the class is the row's argmax
    yo = to_categorical(y, 3)
    _, wc, hc = _fit(w0, x, yo, one_hot=True, class_weight=CW)
    _, wd, hd = _fit(w0, x, yo, one_hot=True, sample_weight=eq)
    assert hc == hd
    for a, b in zip(wc, wd):
        np.testing.assert_array_equal(a, b)
    # both: the product
    _, we, he = _fit(w0, x, y, class_weight=CW, sample_weight=sw)
    _, wf, hf = _fit(w0, x, y, sample_weight=eq * sw)
    assert he == hf
    for a, b in zip(we, wf):
        np.testing.assert_array_equal(a, b)
    # argmax ties go to the smallest index
    tie = np.array([[0.5, 0.5, 0.0], [0.0, 0.4, 0.4], [0.2, 0.2, 0.2]], np.float32)
    np.testing.assert_array_equal(resolve_sample_weights(tie, CW, None, 3), [1.0, 2.5, 1.0])
    out = resolve_sample_weights(y, CW, sw.reshape(-1, 1), 16)
    assert out.dtype == np.float32 and out.shape == (16,) and out.flags["C_CONTIGUOUS"]
    assert resolve_sample_weights(y, None, None, 16) is None


def test_validation_split_and_validation_data():
    w0, x, y, sw = _init_and_data(n=20)
    m, _, h = _fit(w0, x, y, batch=8, sample_weight=sw, validation_split=0.2)
    # the split slices the weights with x and y: training saw the first 16, validation the rest
    _, w16, h16 = _fit(w0, x[:16], y[:16], batch=8, sample_weight=sw[:16])
    for a, b in zip(m.get_weights(), w16):
        np.testing.assert_array_equal(a, b)
    assert h["loss"] == h16["loss"]
    ev = m.evaluate(x[16:], y[16:], batch_size=8, verbose=0, sample_weight=sw[16:], return_dict=True)
    assert h["val_loss"][0] == ev["loss"] and h["val_accuracy"][0] == ev["accuracy"]
    plain = m.evaluate(x[16:], y[16:], batch_size=8, verbose=0, return_dict=True)
    assert plain["loss"] != ev["loss"] and plain["accuracy"] == ev["accuracy"]

    m2, _, h2 = _fit(w0, x[:16], y[:16], batch=8, sample_weight=sw[:16],
                     validation_data=(x[16:], y[16:], sw[16:]))
    assert h2["val_loss"][0] == ev["loss"]
    m3, _, h3 = _fit(w0, x[:16], y[:16], batch=8, sample_weight=sw[:16], validation_data=(x[16:], y[16:]))
    assert h3["val_loss"][0] == plain["loss"]

    # evaluate: the weighted sum over the number of rows; without weights what it always was
    ls, _, corr = _host(m.get_weights(), x[16:], y[16:], sw[16:])
    np.testing.assert_allclose(ev["loss"], float((ls * sw[16:]).sum() / 4), rtol=1e-6)
    np.testing.assert_allclose(plain["loss"], float(ls.mean()), rtol=1e-6)
    got = m.evaluate(x[16:], y[16:], batch_size=8, verbose=0)
    assert got == [plain["loss"], plain["accuracy"]]
    with pytest.raises(ValueError):
        m.evaluate(x[16:], y[16:], verbose=0, sample_weight=sw[:3])


def test_short_final_batch():
    w0, x, y, sw = _init_and_data(n=10)
    # three steps, the last over two rows: gradient scale 1/2, and the epoch's loss is the
    # weighted sum over all batches divided by the 10 rows
    _, w1, h = _fit(w0, x, y, batch=4, sample_weight=sw)
    ws = [w.astype(np.float64) for w in w0]
    total = 0.0
    for lo in (0, 4, 8):
        hi = min(lo + 4, 10)
        ls, grads, _ = _host(ws, x[lo:hi], y[lo:hi], sw[lo:hi])
        total += float((ls * sw[lo:hi]).sum())
        ws = [np.float32(a - LR * g).astype(np.float64) for a, g in zip(ws, grads)]
    np.testing.assert_allclose(h["loss"][0], total / 10, rtol=1e-6)
    for a, b in zip(ws, w1):
        np.testing.assert_allclose(b, a.astype(np.float32), rtol=1e-5, atol=1e-7)


def test_validation_errors():
    w0, x, y, sw = _init_and_data()
    m = _model()
    bad = sw.copy()
    bad[3] = np.nan
    inf = sw.copy()
    inf[3] = np.inf
    for kw, word in ((dict(sample_weight=sw[:15]), "length"),
                     (dict(sample_weight=np.ones((16, 2), np.float32)), "shape"),
                     (dict(sample_weight=bad), "NaN"),
                     (dict(sample_weight=inf), "infinite"),
                     (dict(class_weight={0: 1.0, 2: 2.0}), "keys"),
                     (dict(class_weight={0: 1.0, 1: 2.0}), "label")):
        with pytest.raises(ValueError, match=word):
            m.fit(x, np.where(np.arange(16) == 0, 2, y), batch_size=8, epochs=1, verbose=0, **kw)
    with pytest.raises(ValueError):
        m.fit(x, y, batch_size=8, verbose=0, validation_data=(x, y, sw, sw))


def test_r_mirror():
    w0, x, y, sw = _init_and_data()
    y2 = y % 2
    a = _model()
    a.set_weights(w0)
    ha = r_api.fit(a, x, y2, batch_size=8, epochs=1, shuffle=False, verbose=0, class_weight={"0": 1, "1": 2},
                   sample_weight=sw)
    b = _model()
    b.set_weights(w0)
    hb = b.fit(x, y2, batch_size=8, epochs=1, shuffle=False, verbose=0, class_weight={0: 1, 1: 2}, sample_weight=sw)
    assert ha.history == hb.history
    for u, v in zip(a.get_weights(), b.get_weights()):
        np.testing.assert_array_equal(u, v)
    assert r_api.evaluate(a, x, y2, batch_size=8, verbose=0, sample_weight=sw) == \
        b.evaluate(x, y2, batch_size=8, verbose=0, sample_weight=sw)
    with pytest.raises(ValueError):
        r_api.fit(a, x, y2, batch_size=8, epochs=1, verbose=0, class_weight={"a": 1, "b": 2})


def test_fused_engine_eligibility_and_engine_key():
    class _FakeGPUStrategy:
        device = torch.device("cuda")

    keras.backend.clear_session()
    m = keras.Sequential([L.Conv2D(32, 3, activation="relu", input_shape=(28, 28, 1)), L.MaxPooling2D(),
                          L.Flatten(), L.Dense(64, activation="relu"), L.Dense(10)])
    m.compile(optimizer=O.SGD(0.01), loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True),
              metrics=["accuracy"])
    st = _FakeGPUStrategy()
    assert FusedConvNetEngine.eligible(m, st) == (True, "")
    assert FusedConvNetEngine.eligible(m, st, weighted=False) == (True, "")
    assert FusedConvNetEngine.eligible(m, st, weighted=True) == (False, "sample weights")
    assert NativeGraphEngine.eligible(m, st) == (True, "")
    # the engine cache tells a weighted fit from an unweighted one
    w0, x, y, sw = _init_and_data()
    d = _model()
    d.fit(x, y, batch_size=8, epochs=1, verbose=0)
    e0 = d._engine
    d.fit(x, y, batch_size=8, epochs=1, verbose=0)
    assert d._engine is e0
    d.fit(x, y, batch_size=8, epochs=1, verbose=0, sample_weight=sw)
    e1 = d._engine
    assert e1 is not e0 and e1.feed.w is not None
    d.fit(x, y, batch_size=8, epochs=1, verbose=0)
    assert d._engine is not e1 and d._engine.feed.w is None


# --- world 2 over gloo ---------------------------------------------------------------------------
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
    assert set(w0) == set(w1) == set(ws) and len(w0) == 12
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k  # replicas stay bitwise mirrored
        # the bounds of tests/test_grad_clipping.py::test_world_2_matches_world_1
        np.testing.assert_allclose(w0[k], ws[k], rtol=1e-4, atol=1e-6, err_msg=k)
    assert j0["runs"] == j1["runs"]
    for name in ("none", "sample", "both"):
        assert j0["runs"][name]["iterations"] == js["runs"][name]["iterations"] == 6
        np.testing.assert_allclose(j0["runs"][name]["loss"], js["runs"][name]["loss"], rtol=1e-5)
        np.testing.assert_allclose(j0["runs"][name]["accuracy"], js["runs"][name]["accuracy"], rtol=1e-6)
    for name in ("sample", "both"):  # the weights really acted
        assert any(not np.array_equal(ws[f"{name}/{i}"], ws[f"none/{i}"]) for i in range(4)), name
    assert any(not np.array_equal(ws[f"sample/{i}"], ws[f"both/{i}"]) for i in range(4))
