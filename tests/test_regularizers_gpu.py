"""Weight regularizers on the GPU: the opt_step kernel with a segment table and the
reg_penalty reduction against the fp32 / fp64 host references, and whole native-engine
training runs (loss, update, evaluate, graph replay, per-bucket updates, short batches,
BatchNorm variables) against the closed form and the generic engine."""
import struct

import numpy as np
import pytest
import torch

import distributed_amd as tf
from distributed_amd.engine.ctrl import C_CUR3, C_IT, C_LR
from distributed_amd.ops import hip as H
from distributed_amd.ops import reference as R

from test_native_graph_gpu import _data, _mnist, _train

pytestmark = pytest.mark.gpu
dev = "cuda"
REG, L = tf.keras.regularizers, tf.keras.layers

# five variables at 8-aligned offsets of a flat buffer: padding gaps, a variable shorter than
# one vector, one spanning several blocks; (l1 only), (no row), (l2 only), (both), (no row)
SIZES = (1, 7, 8, 1000, 4099)
COEF = ((0.03, 0.0), None, (0.0, 0.2), (0.02, 0.05), None)


def _layout(sizes=SIZES, coef=COEF):
    offs, off = [], 0
    for sz in sizes:
        offs.append(off)
        off = -(-(off + sz) // 8) * 8
    rows = [(o, sz, c[0], c[1]) for o, sz, c in zip(offs, sizes, coef) if c is not None]
    return offs, off, rows


def _flat(seed, offs, n, sizes=SIZES, scale=1.0, zeros=True):
    """Values on the variables (every fifth an exact zero), zero padding."""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(n)
    for o, sz in zip(offs, sizes):
        v = torch.randn(sz, generator=g) * scale
        if zeros:
            v[::5] = 0.0
        p[o:o + sz] = v
    return p


def _i(f):
    return struct.unpack("<i", struct.pack("<f", float(f)))[0]


def _opt_cases():
    O = tf.keras.optimizers
    return {"sgd_nesterov": lambda: O.SGD(learning_rate=0.05, momentum=0.9, nesterov=True),
            "adam": lambda: O.Adam(learning_rate=1e-3),
            "rmsprop_momentum": lambda: O.RMSprop(learning_rate=5e-4, momentum=0.9)}


class _Flat:
    """Device state of one opt_step sequence."""

    def __init__(self, p0, opt):
        from distributed_amd.engine.native_graph import _opt_kernel_slots
        from distributed_amd.native import require_C

        self.C, self.n = require_C(), p0.numel()
        self.kind, self.names = _opt_kernel_slots(opt)
        self.P = p0.clone().to(dev)
        self.Pb = torch.zeros(self.n, dtype=torch.bfloat16, device=dev)
        self.S = [torch.zeros(self.n, device=dev) for _ in range(3)]
        self.ctrl = torch.zeros(32, dtype=torch.int32, device=dev)
        self.ctrl[C_LR] = _i(opt.learning_rate)
        self.tail = torch.zeros(8, device=dev)
        if self.kind == 1:
            self.args = (opt.beta_1, opt.beta_2, opt.epsilon, 0.0, 0.0, int(opt.amsgrad))
        elif self.kind == 2:
            self.args = (0.0, 0.0, opt.epsilon, opt.rho, opt.momentum, int(opt.centered))
        else:
            self.args = (0.0, 0.0, 0.0, 0.0, opt.momentum, int(opt.nesterov))

    def step(self, t, g, table=None, splits=None):
        """One optimizer step with gradient g; splits: launch boundaries (element offsets)."""
        self.ctrl[C_CUR3] = t
        G = g.to(dev)
        cuts = [0] + list(splits or []) + [self.n]
        for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            kw = {}
            if table is not None:
                kw = dict(reg=table.data_ptr(), nreg=table.shape[0], lo=lo)
            self.C.opt_step(self.P.data_ptr() + 4 * lo, G.data_ptr() + 4 * lo, *(s.data_ptr() + 4 * lo for s in self.S),
                            self.Pb.data_ptr() + 2 * lo, hi - lo, self.ctrl.data_ptr(), self.tail.data_ptr(), self.kind,
                            *map(float, self.args[:5]), self.args[5], torch.cuda.current_stream().cuda_stream,
                            book=int(k == len(cuts) - 2), **kw)
        torch.cuda.synchronize()

    def state(self):
        return [self.P.cpu().numpy(), self.Pb.float().cpu().numpy()] + [s.cpu().numpy() for s in self.S]


@pytest.mark.parametrize("name", list(_opt_cases()))
def test_opt_step_with_table_matches_reference(name):
    """opt_step with the segment table against reg_grad + the Keras optimizer's own fp32
    apply_flat on the CPU, three steps; the split launch and the all-zero table bitwise."""
    offs, n, rows = _layout()
    table = H.reg_table(rows, dev)
    assert tuple(table.shape) == (3, 4)
    p0 = _flat(1, offs, n)
    opt_h = _opt_cases()[name]()
    opt_h.ensure_slots(n, torch.device("cpu"))
    ph = p0.clone()
    one, two = _Flat(p0, _opt_cases()[name]()), _Flat(p0, _opt_cases()[name]())
    for t in range(1, 4):
        g = _flat(10 + t, offs, n, scale=0.1 if t % 2 else 1.0, zeros=False)
        one.step(t, g, table)
        two.step(t, g, table, splits=[offs[2]])  # pointers advanced, absolute lo passed
        opt_h.apply_flat(ph, g + R.reg_grad(ph, rows))
        torch.testing.assert_close(one.P.cpu(), ph, rtol=1e-5, atol=1e-6)
        assert int(one.ctrl[C_IT]) == t and int(two.ctrl[C_IT]) == t
        for i, nm in enumerate(one.names):
            if nm:
                torch.testing.assert_close(one.S[i].cpu(), opt_h.slots[nm], rtol=1e-5, atol=1e-7)
        for a, b in zip(one.state(), two.state()):
            assert a.tobytes() == b.tobytes()  # two launches == one launch, bitwise
    assert torch.equal(one.Pb, one.P.bfloat16())
    # an all-zero-coefficient table == the launch without a table
    zero = H.reg_table([(o, sz, 0.0, 0.0) for o, sz, _, _ in rows], dev)
    a, b = _Flat(p0, _opt_cases()[name]()), _Flat(p0, _opt_cases()[name]())
    for t in range(1, 3):
        g = _flat(20 + t, offs, n, zeros=False)
        a.step(t, g, zero)
        b.step(t, g)
    for x, y in zip(a.state(), b.state()):
        np.testing.assert_array_equal(x, y)


def test_reg_table_checks():
    with pytest.raises(ValueError):
        H.reg_table([(4, 8, 0.1, 0.0)], dev)  # offset not on an 8-element boundary
    with pytest.raises(ValueError):
        H.reg_table([(0, 16, 0.1, 0.0), (8, 8, 0.1, 0.0)], dev)  # overlap
    with pytest.raises(ValueError):
        H.reg_table([(8 * i, 8, 0.1, 0.0) for i in range(H.REG_MAX_ROWS + 1)], dev)
    from distributed_amd.native import require_C

    assert require_C().REG_MAX_ROWS == H.REG_MAX_ROWS


def _host_penalty(p, rows):
    p = p.double().numpy()
    return sum(l1 * np.abs(p[o:o + sz]).sum() + l2 * (p[o:o + sz] ** 2).sum() for o, sz, l1, l2 in rows)


# the second layout: more groups than 1024 blocks x 256 threads x 4 (the grid's cap: several
# groups per thread, 1075 per block), rows ending inside a block
@pytest.mark.parametrize("sizes,coef", [(SIZES, COEF), ((3_000_001, 13, 1_400_003), ((0.01, 0.02), None, (0.0, 0.3)))],
                         ids=["small", "capped_grid"])
def test_reg_penalty(sizes, coef):
    """R against the fp64 host value (rtol 1e-5: each thread adds < 64 fp32 terms and the
    trees add ~14 levels, ~5e-6), the tail update, and bitwise repeatability."""
    offs, n, rows = _layout(sizes, coef)
    table = H.reg_table(rows, dev)
    p = _flat(4, offs, n, sizes)
    want = _host_penalty(p, rows)
    np.testing.assert_allclose(float(R.reg_penalty(p, rows)), want, rtol=1e-5)  # the fp32 reference itself
    P = p.to(dev)
    scratch = H.reg_scratch(n, dev)
    if n > 2 ** 22:
        assert scratch.numel() == 1024 + 2
    preset = [3.5, 7.0, 24.0, 9.0, -1.0, 0.25, 2.0, 11.0]
    tail = torch.tensor(preset, device=dev)
    H.reg_penalty(P, table, scratch, tail=tail)
    torch.cuda.synchronize()
    r1 = scratch[-1].item()
    np.testing.assert_allclose(r1, want, rtol=1e-5)
    t = tail.cpu().numpy()
    np.testing.assert_allclose(t[0], np.float32(preset[0]) + np.float32(r1) * np.float32(24.0), rtol=1e-6)
    np.testing.assert_array_equal(t[1:], np.float32(preset[1:]))
    assert int(scratch[-2:-1].view(torch.int32)) == 0  # the arrival counter re-armed
    H.reg_penalty(P, table, scratch, tail=tail)  # the same scratch: the same bits
    torch.cuda.synchronize()
    assert struct.pack("<f", scratch[-1].item()) == struct.pack("<f", r1)
    np.testing.assert_allclose(tail[0].item(), np.float32(preset[0]) + 2 * np.float32(r1) * np.float32(24.0), rtol=1e-6)
    H.reg_penalty(P, table, scratch)  # no tail: R only
    torch.cuda.synchronize()
    assert struct.pack("<f", scratch[-1].item()) == struct.pack("<f", r1)
    # a table without rows: tail[0] unchanged, R = 0
    before = tail.clone()
    H.reg_penalty(P, H.reg_table([], dev), scratch, tail=tail)
    torch.cuda.synchronize()
    assert torch.equal(tail, before) and scratch[-1].item() == 0.0


# --- the native engine end to end ---------------------------------------------------------------
LR = 0.05


def _reg_mnist():
    return tf.keras.Sequential([
        L.Conv2D(32, 3, activation="relu", input_shape=(28, 28, 1), kernel_regularizer=REG.l2(0.05)),
        L.MaxPooling2D(),
        L.Flatten(),
        L.Dense(64, activation="relu", kernel_regularizer=REG.l2(0.05), bias_regularizer=REG.l1(0.01)),
        L.Dense(10, kernel_regularizer=REG.l2(0.05)),
    ])


# (index into get_weights(), l1, l2) of the regularized variables of _reg_mnist
MNIST_REGS = ((0, 0.0, 0.05), (2, 0.0, 0.05), (3, 0.01, 0.0), (4, 0.0, 0.05))
STRICT = {"DAMD_STRICT_NATIVE": "1"}


def _penalty(ws, regs):
    return sum(l1 * np.abs(ws[i].astype(np.float64)).sum() + l2 * (ws[i].astype(np.float64) ** 2).sum()
               for i, l1, l2 in regs)


@pytest.fixture(scope="module")
def mnist_case():
    tf.set_seed(7)
    tf.keras.backend.clear_session()
    init = _mnist().get_weights()
    rng = np.random.default_rng(2)
    init[3] = rng.normal(0, 0.05, init[3].shape).astype(np.float32)  # dense bias: L1 needs non-zeros ...
    init[3][::7] = 0.0  # ... and exact zeros (sign(0) = 0)
    x, y = _data(96, (28, 28, 1), 10)
    return init, x, y


def _native(build, x, y, init, steps, fused, **env):
    w, h, eng = _train(build, x, y, init, 32, steps, native=True, lr=LR, fused=fused, extra_env={**STRICT, **env})
    assert eng == "native_graph", eng
    return w, h


def test_native_step_matches_closed_form_and_generic(mnist_case):
    init, x, y = mnist_case
    # the regularized model under DAMD_FUSED=1 must land on native_graph (the fused MNIST
    # engine rejects it); the plain one is kept off the fused engine
    wr, hr = _native(_reg_mnist, x, y, init, 1, fused=True)
    wp, hp = _native(_mnist, x, y, init, 1, fused=False)
    for i, l1, l2 in MNIST_REGS:
        w0 = init[i].astype(np.float64)
        want = -LR * (2 * l2 * w0 + l1 * np.sign(w0))
        np.testing.assert_allclose(wr[i].astype(np.float64) - wp[i], want, atol=1e-6, rtol=0)
    np.testing.assert_array_equal(wr[1], wp[1])  # the conv bias carries no regularizer
    zero = init[3] == 0.0
    np.testing.assert_array_equal(wr[3][zero], wp[3][zero])
    R0 = _penalty(init, MNIST_REGS)
    print(f"R(w0) = {R0:.6f}, loss {hr['loss'][0]:.6f} vs plain {hp['loss'][0]:.6f}")
    np.testing.assert_allclose(hr["loss"][0] - hp["loss"][0], R0, rtol=1e-4)
    assert hr["accuracy"] == hp["accuracy"]
    # three steps track the generic engine on the CPU
    w3, h3 = _native(_reg_mnist, x, y, init, 3, fused=True)
    wg, hg, eng = _train(_reg_mnist, x, y, init, 32, 3, native=False, lr=LR, device="cpu")
    assert eng == "generic"
    print("3 steps: native", h3["loss"], "generic", hg["loss"])
    np.testing.assert_allclose(h3["loss"], hg["loss"], rtol=1e-2)


def test_native_evaluate_includes_penalty(mnist_case, monkeypatch):
    from distributed_amd.parallel import runtime

    init, x, y = mnist_case
    for k, v in {**STRICT, "DAMD_FUSED": "1", "DAMD_NATIVE_GRAPH": "1"}.items():
        monkeypatch.setenv(k, v)
    runtime.shutdown()
    out = {}
    try:
        for name, build in (("reg", _reg_mnist), ("plain", _mnist)):
            tf.keras.backend.clear_session()
            m = build()
            m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=tf.keras.optimizers.SGD(LR), metrics=["accuracy"])
            m.set_weights(init)
            out[name] = m.evaluate(x[:72], y[:72], batch_size=32, verbose=0)  # a short last batch
            assert m.__dict__["_infer_plans"], "evaluate did not go through the native plan"
            if name == "reg":
                np.testing.assert_allclose([float(t) for t in m.losses],
                                           [_penalty(init, [r]) for r in MNIST_REGS], rtol=1e-5)
    finally:
        runtime.shutdown()
    np.testing.assert_allclose(out["reg"][0] - out["plain"][0], _penalty(init, MNIST_REGS), rtol=1e-4)
    assert out["reg"][1] == out["plain"][1]


def test_replay_and_buckets_are_bitwise(mnist_case):
    init, x, y = mnist_case
    base, hb = _native(_reg_mnist, x[:64], y[:64], init, 4, fused=True)
    eager, he = _train(_reg_mnist, x[:64], y[:64], init, 32, 4, native=True, lr=LR, fused=True, graph=False,
                       extra_env=STRICT)[:2]
    for a, b in zip(base, eager):
        np.testing.assert_array_equal(a, b)
    assert hb == he
    # several per-bucket opt_step launches (each with its absolute offset) == the single launch
    bucketed, _ = _native(_reg_mnist, x[:64], y[:64], init, 4, fused=True, DAMD_BUCKET_OPT="1", DAMD_BUCKET_MB="0.05")
    for a, b in zip(base, bucketed):
        np.testing.assert_array_equal(a, b)


def test_short_final_batch(mnist_case):
    """n = 40 at batch 32: the epoch loss is sum n_t (L_t + R_t) / 40 with R_t at the weights
    step t's forward used."""
    init, x, y = mnist_case
    x, y = x[:40], y[:40]
    w2, h2 = _native(_reg_mnist, x, y, init, None, fused=True)
    wg, hg, _ = _train(_reg_mnist, x, y, init, 32, None, native=False, lr=LR, device="cpu")
    print("short batch: native", h2["loss"], "generic", hg["loss"])
    np.testing.assert_allclose(h2["loss"], hg["loss"], rtol=1e-2)
    # the plain native data losses at the same weights + the host-computed penalties:
    # step 1 from w0 on rows 0..31, step 2 from the regularized run's w1 on rows 32..39
    w1, _ = _native(_reg_mnist, x[:32], y[:32], init, 1, fused=True)
    _, p1 = _native(_mnist, x[:32], y[:32], init, 1, fused=False)
    _, p2 = _native(_mnist, x[32:], y[32:], w1, None, fused=False)
    want = (32 * (p1["loss"][0] + _penalty(init, MNIST_REGS)) + 8 * (p2["loss"][0] + _penalty(w1, MNIST_REGS))) / 40
    print(f"epoch loss {h2['loss'][0]:.6f}, data losses + penalties {want:.6f}")
    np.testing.assert_allclose(h2["loss"][0], want, rtol=1e-4)


def _bn_net(reg):
    def build():
        kw = dict(gamma_regularizer=REG.l2(0.1), beta_regularizer=REG.l1(0.05)) if reg else {}
        return tf.keras.Sequential([L.Conv2D(8, 3, use_bias=False, padding="same", input_shape=(8, 8, 8)),
                                    L.BatchNormalization(**kw), L.ReLU(), L.GlobalAveragePooling2D(), L.Dense(10)])
    return build


def test_batchnorm_variables():
    tf.set_seed(9)
    tf.keras.backend.clear_session()
    init = _bn_net(False)().get_weights()  # conv kernel, gamma, beta, moving mean, moving variance, dense kernel, bias
    rng = np.random.default_rng(6)
    init[1] = (1.0 + rng.normal(0, 0.2, 8)).astype(np.float32)
    init[2] = rng.normal(0, 0.3, 8).astype(np.float32)
    init[2][3] = 0.0
    x, y = _data(32, (8, 8, 8), 10, seed=3)
    wr, hr = _native(_bn_net(True), x, y, init, 1, fused=True)
    wp, hp = _native(_bn_net(False), x, y, init, 1, fused=True)
    for i, l1, l2 in ((1, 0.0, 0.1), (2, 0.05, 0.0)):
        w0 = init[i].astype(np.float64)
        np.testing.assert_allclose(wr[i].astype(np.float64) - wp[i], -LR * (2 * l2 * w0 + l1 * np.sign(w0)),
                                   atol=1e-6, rtol=0)
    assert wr[2][3] == wp[2][3]
    for i in (0, 3, 4, 5, 6):  # the conv kernel's update (and everything else) is the plain run's, bitwise
        np.testing.assert_array_equal(wr[i], wp[i])
    np.testing.assert_allclose(hr["loss"][0] - hp["loss"][0], _penalty(init, ((1, 0.0, 0.1), (2, 0.05, 0.0))),
                               rtol=1e-4)
