"""The constant-configuration MNIST step kernels (fwd_flag / bwd_flag, convnet_step2.hip:
world 1, 64 images, default slicing, eager W1 update) against the generic kernels of the
same build (DAMD_SPECIALISED=0): the same bits, and the dispatch between the two."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FEAT, HID = 5408, 64


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _model(lr=0.1, momentum=0.0, nesterov=False, seed=3):
    import distributed_amd as tf

    tf.set_seed(seed)
    m = tf.models.mnist_cnn()
    m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
              optimizer=tf.keras.optimizers.SGD(learning_rate=lr, momentum=momentum, nesterov=nesterov),
              metrics=["accuracy"])
    return m


def _data(n, seed=0, u8=True):
    """u8: inputs that are exactly k / 255 (kept as uint8 rows on the device)."""
    rng = np.random.default_rng(seed)
    if u8:
        x = rng.integers(0, 256, (n, 28, 28, 1)).astype(np.uint8) / 255.0
    else:
        x = rng.random((n, 28, 28, 1), dtype=np.float32)
    y = rng.integers(0, 10, n).astype(np.int64)
    return x, y


def _engine(model, B):
    eng = model._get_engine(B, B)
    assert eng.name == "fused_convnet", "fused engine must be selected on GPU"
    return eng


def _flat(m):
    return np.concatenate([w.ravel() for w in m.get_weights()])


def _arms(monkeypatch, run, **model_kw):
    """run(engine) -> list of metric dicts, once per arm; returns per arm (initial weights,
    final weights, metrics), after checking which kernels each arm ran."""
    out = []
    for spec in ("1", "0"):
        monkeypatch.setenv("DAMD_SPECIALISED", spec)
        m = _model(**model_kw)
        w0 = [w.copy() for w in m.get_weights()]
        eng = _engine(m, 64)
        assert eng.step_kernels == ("specialised" if spec == "1" else "generic")
        mets = run(eng)
        eng.finish()
        out.append((w0, [w.copy() for w in m.get_weights()], mets))
    return out


def _assert_same_bits(arms):
    (_, wa, ma), (_, wb, mb) = arms
    for a, b in zip(wa, wb):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert ma == mb, (ma, mb)
    assert all(np.isfinite(mt["loss"]) for mt in ma), ma


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, True)], ids=["sgd", "nesterov"])
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "fp32"])
def test_specialised_equals_generic_bitwise(u8, momentum, nesterov, graph, monkeypatch):
    """6 steps from the same seed (both step parities twice), eager launches or a captured
    3-step graph replayed twice: every weight and the epoch metrics are the same bits."""
    _need_gpu()
    monkeypatch.setenv("DAMD_X_U8", "1" if u8 else "0")
    monkeypatch.setenv("DAMD_GRAPH", "1" if graph else "0")
    monkeypatch.setenv("DAMD_GRAPH_STEPS", "3")
    x, y = _data(64 * 6, u8=u8)

    def run(eng):
        eng.bind(x, y)
        assert eng.feed.x_u8 == u8
        eng.start_epoch(0, shuffle=True)
        if graph:
            eng.prepare(3)
        eng.run(6)
        if graph:
            assert eng.trainer.num_graphs >= 1
        return [eng.end_epoch()]

    _assert_same_bits(_arms(monkeypatch, run, lr=0.05, momentum=momentum, nesterov=nesterov, seed=11))


def test_short_last_batch_and_epoch_flush_bitwise(monkeypatch):
    """64 * 3 + 17 rows, 2 epochs of 4 steps: the invalid rows of the last batch, the epoch
    change (new rows: the prefetched batch must miss) and the flush between the epochs."""
    _need_gpu()
    monkeypatch.setenv("DAMD_GRAPH", "0")
    x, y = _data(64 * 3 + 17, seed=5)

    def run(eng):
        eng.bind(x, y)
        mets = []
        for ep in range(2):
            eng.start_epoch(ep, shuffle=True)
            eng.run(4)
            mets.append(eng.end_epoch())
        assert mets[0]["_count"] == 64 * 3 + 17
        return mets

    _assert_same_bits(_arms(monkeypatch, run, lr=0.05, momentum=0.9, seed=13))


def test_short_last_slice_is_updated(monkeypatch):
    """The last slice of either grid holds one pooled position (168) where the others hold 3
    (fwd) / 2 (bwd): after one step its 32 feature rows of W1 and the conv parameters have
    changed, and are the same bits in both arms -- a dropped short slice cannot hide."""
    _need_gpu()
    monkeypatch.setenv("DAMD_GRAPH", "0")
    x, y = _data(64, seed=9)

    def run(eng):
        eng.bind(x, y)
        eng.start_epoch(0, shuffle=False)
        eng.run(1)
        return [eng.end_epoch()]

    arms = _arms(monkeypatch, run, lr=0.5, seed=7)
    for w0, w1, _ in arms:
        last0, last1 = w0[2][FEAT - 32:], w1[2][FEAT - 32:]
        assert last0.shape == (32, HID)
        # its rows moved: all but those of a channel whose ReLU output is 0 for every image
        # (the row's gradient is then exactly 0) -- the same channels as at position 167,
        # whose windows see inputs of the same distribution; a dropped slice moves none
        moved = np.abs(last1 - last0).max(axis=1) > 0
        prev = np.abs(w1[2][FEAT - 64:FEAT - 32] - w0[2][FEAT - 64:FEAT - 32]).max(axis=1) > 0
        assert moved.sum() >= 16 and prev.sum() >= 16, (moved.sum(), prev.sum())
        assert np.abs(w1[0] - w0[0]).max() > 0 and np.abs(w1[1] - w0[1]).max() > 0
    _assert_same_bits(arms)
    assert np.array_equal(arms[0][1][2][FEAT - 32:], arms[1][1][2][FEAT - 32:])


# ---- dispatch --------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _ref_step(ws, xb, yb, gcount, quant=False):
    """fp64 torch reference of one step: (grads, loss_sum, correct); quant=True mirrors the
    kernels' bf16 quantisation points (pooled activations and W1 into dense-1)."""
    from distributed_amd.ops import reference as R

    ts = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in ws]
    x = torch.tensor(xb, dtype=torch.float64)
    h = torch.relu(R.conv2d(x, ts[0], ts[1]))
    p = R.maxpool2d(h)
    f = p.reshape(p.shape[0], -1)
    w1 = ts[2]
    if quant:
        f = f + (_bf16(f) - f).detach()
        w1 = w1 + (_bf16(w1) - w1).detach()
    d = torch.relu(f @ w1 + ts[3])
    z = d @ ts[4] + ts[5]
    ls = torch.nn.functional.cross_entropy(z, torch.tensor(yb), reduction="none")
    (ls.sum() / gcount).backward()
    corr = float((z.argmax(-1) == torch.tensor(yb)).sum())
    return [t.grad.numpy() for t in ts], float(ls.detach().sum()), corr


def _one_step_vs_reference(B, expect):
    """One step against the fp32-model reference, with the bounds of
    tests/test_fused_convnet_gpu.py (60-draw sweep, scripts/sweep_fused_ref.py)."""
    lr = 0.5
    m = _model(lr=lr, seed=3)
    rng = np.random.default_rng(0)
    x = rng.random((300, 28, 28, 1), dtype=np.float32)
    y = rng.integers(0, 10, 300).astype(np.int64)
    w0 = m.get_weights()
    eng = _engine(m, B)
    assert eng.step_kernels == expect
    eng.bind(x, y)
    eng.start_epoch(0, shuffle=False)
    eng.run(1)
    met = eng.end_epoch()
    eng.finish()
    w1 = m.get_weights()
    names = ["wc", "bc", "w1", "b1", "w2", "b2"]

    def rel_errs(grads):
        out, cols = {}, {}
        for a, b, g, name in zip(w0, w1, grads, names):
            est = (a - b) / lr
            out[name] = float(np.linalg.norm(est - g) / (np.linalg.norm(g) + 1e-12))
            E, G = est.reshape(-1, est.shape[-1]), g.reshape(-1, g.shape[-1])
            ce = np.linalg.norm(E - G, axis=0) / (np.linalg.norm(G, axis=0) + 1e-12)
            cols[name] = float((ce < 1e-2).mean())
        return out, cols

    gq, lsum, corr = _ref_step(w0, x[:B], y[:B], B, quant=True)
    eq, cq = rel_errs(gq)
    print("vs bf16-mirrored reference:", {k: f"{v:.2e}" for k, v in eq.items()}, "columns within 1e-2:", cq)
    assert cq["w1"] >= 0.95 and cq["b1"] >= 0.95, cq
    assert eq["w2"] < 5e-3 and eq["b2"] < 5e-3, eq
    assert max(eq.values()) < 0.1, eq
    g64, _, _ = _ref_step(w0, x[:B], y[:B], B, quant=False)
    e64, _ = rel_errs(g64)
    print("vs fp64 reference:", {k: f"{v:.2e}" for k, v in e64.items()})
    assert max(e64.values()) < 0.2, e64
    assert abs(met["loss"] - lsum / B) < 2e-2
    assert abs(met["accuracy"] - corr / B) < 1.5 / B


@pytest.mark.parametrize("B,env,expect", [
    (64, {}, "specialised"),
    (32, {}, "generic"),
    (64, {"DAMD_PP": "2"}, "generic"),
    (64, {"DAMD_EAGER_W1": "0"}, "generic"),
], ids=["default", "B32", "PP2", "deferred"])
def test_dispatch_and_reference(B, env, expect, monkeypatch):
    """The default configuration runs the specialised kernels; another batch, another fwd
    slicing or the deferred update run the generic ones -- and each still matches the
    reference step."""
    _need_gpu()
    monkeypatch.setenv("DAMD_GRAPH", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _one_step_vs_reference(B, expect)
