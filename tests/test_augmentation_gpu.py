"""Input augmentation on the GPU: the ``augment`` kernel against the host oracle (bitwise), the
native graph engine's fresh draws per step with and without graph replay, its bitwise
equivalence to training on oracle-augmented data, and native inference behind a prefix."""
import logging
import os

import numpy as np
import pytest
import torch

import distributed_amd as tf
from distributed_amd.engine.ctrl import C_CUR3, C_ROW0
from distributed_amd.ops import hip as H

pytestmark = pytest.mark.gpu
L = tf.keras.layers

F3, F1, F2 = (H.AUG_FLIP, 3, 0, 0, 0, 0x1234), (H.AUG_FLIP, 1, 0, 0, 0, 77), (H.AUG_FLIP, 2, 0, 0, 0, 78)
STAGE_LISTS = {
    "hflip": [F1],
    "both_flips": [F3],
    "pad_crop_flip": [(H.AUG_PAD, 1, 2, 3, 0, 0), (H.AUG_CROP, 4, 6, 0, 0, 99), F3],
    # crop 3x5 -> pad to 6x8 -> crop 5x6: a zero band of the pad lies inside the final window
    "crop_pad_crop": [(H.AUG_CROP, 3, 5, 0, 0, 5), (H.AUG_PAD, 2, 1, 1, 2, 0), (H.AUG_CROP, 5, 6, 0, 0, 6)],
    "eight": [F1, (H.AUG_PAD, 1, 1, 1, 1, 0), (H.AUG_CROP, 6, 8, 0, 0, 1), F2, (H.AUG_CROP, 4, 5, 0, 0, 2),
              (H.AUG_PAD, 0, 2, 3, 0, 0), F3, (H.AUG_CROP, 5, 7, 0, 0, 3)],
}


def _out_hw(stages, h, w):
    for k, p0, p1, p2, p3, _ in stages:
        if k == H.AUG_CROP:
            h, w = p0, p1
        elif k == H.AUG_PAD:
            h, w = h + p0 + p1, w + p2 + p3
    return h, w


def _ctrl(t, row0):
    c = torch.zeros(32, dtype=torch.int32)
    c[C_ROW0], c[C_CUR3] = row0, t
    return c.cuda()


@pytest.fixture(scope="module")
def images():
    """{Cp: (uint16 bit patterns [3, 5, 7, Cp] on the host, the same as a bf16 device tensor)}:
    every 16-bit pattern distinct and non-zero, so the comparison is on bits, NaNs included."""
    out = {}
    for cp in (4, 8, 24):
        bits = (np.random.default_rng(cp).permutation(3 * 5 * 7 * cp) + 1).astype(np.uint16).reshape(3, 5, 7, cp)
        out[cp] = (bits, torch.from_numpy(bits.view(np.int16)).cuda().view(torch.bfloat16))
    return out


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", list(STAGE_LISTS))
@pytest.mark.parametrize("cp", [4, 8, 24])
def test_kernel_equals_the_oracle_bitwise(images, cp, name, training):
    stages = STAGE_LISTS[name]
    bits, x = images[cp]
    ho, wo = _out_hw(stages, 5, 7)
    tab = H.aug_table(stages)
    labels = torch.zeros(3, dtype=torch.int32, device="cuda")
    for t in (1, 2, 1000003):
        for row0 in (0, 3):
            y = torch.full((3, ho, wo, cp), 1.0, dtype=torch.bfloat16, device="cuda")
            H.augment(x, y, labels, _ctrl(t, row0), tab, training)
            got = y.view(torch.int16).cpu().numpy().view(np.uint16)
            ref = H.augment_reference(bits, stages, t, row0, training)
            assert ref.shape == got.shape
            assert np.array_equal(got, ref), (cp, name, training, t, row0)


def test_invalid_row_is_zero(images):
    bits, x = images[8]
    stages = STAGE_LISTS["pad_crop_flip"]
    y = torch.full((3, 4, 6, 8), 1.0, dtype=torch.bfloat16, device="cuda")
    labels = torch.tensor([0, -1, 5], dtype=torch.int32, device="cuda")
    H.augment(x, y, labels, _ctrl(2, 0), H.aug_table(stages), True)
    got = y.view(torch.int16).cpu().numpy().view(np.uint16)
    ref = H.augment_reference(bits, stages, 2, 0, True)
    assert not got[1].any() and ref[1].any()
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])


def test_bad_arguments_launch_nothing(images):
    bits, x = images[8]
    labels = torch.zeros(3, dtype=torch.int32, device="cuda")
    ctrl = _ctrl(1, 0)
    good = H.aug_table(STAGE_LISTS["pad_crop_flip"])

    def out(h=4, w=6, cp=8):
        return torch.full((3, h, w, cp), 1.0, dtype=torch.bfloat16, device="cuda")

    def untouched(y):
        torch.cuda.synchronize()
        return bool((y.float() == 1.0).all())

    C = H._C()

    def raw(x_, y_, tab, B=3, h=5, w=7, ho=4, wo=6, cp=8, lab=labels, c=ctrl):
        C.augment(H._ptr(x_), H._ptr(y_), H._ptr(lab), H._ptr(c), tab.data_ptr() if tab is not None else 0, B, h, w,
                  ho, wo, cp, 1, H.stream_handle())

    def edited(word, value):
        t = good.clone()
        t[word] = value
        return t

    y = out()
    # words: 4 of header, then 8 per stage (kind, p0 .. p3, seed): pad, crop, flip
    bad_tabs = [edited(0, 0), edited(0, 9),  # no stage / beyond the cap
                edited(4 + 8, 7),  # unknown kind
                edited(4 + 8 + 1, 9),  # crop taller than its input
                edited(4 + 1, -1),  # negative pad
                edited(4 + 16 + 1, 0)]  # flip without an axis
    for t in bad_tabs:
        with pytest.raises(RuntimeError, match="augment"):
            raw(x, y, t)
    for kw in (dict(ho=5), dict(wo=7), dict(cp=6), dict(cp=0), dict(B=0), dict(B=70000)):
        with pytest.raises(RuntimeError, match="augment"):  # shapes the table does not lead to / bad pitch
            raw(x, y, good, **kw)
    with pytest.raises(RuntimeError, match="augment"):
        raw(x, y, None)
    with pytest.raises(RuntimeError, match="augment"):
        raw(x, y, good, lab=None)
    with pytest.raises(RuntimeError, match="augment"):
        raw(x, y, good, c=None)
    with pytest.raises(RuntimeError, match="augment"):
        raw(None, y, good)
    with pytest.raises(RuntimeError, match="augment"):
        raw(x, x, good, ho=5, wo=7)  # in place
    assert untouched(y)
    # the launcher's own checks
    with pytest.raises(TypeError):
        H.augment(x.float(), y, labels, ctrl, good, True)
    with pytest.raises(ValueError):
        H.augment(x, out(cp=16), labels, ctrl, good, True)
    with pytest.raises(ValueError):
        H.augment(x, y, labels, ctrl, good.cuda(), True)
    with pytest.raises(ValueError):
        H.augment(x, y, labels[:2], ctrl, good, True)
    with pytest.raises(RuntimeError, match="augment"):
        H.augment(x, out(5, 6), labels, ctrl, good, True)
    assert untouched(y)
    H.augment(x, y, labels, ctrl, good, True)  # and the good call still works
    assert not untouched(y)


# --- the engines -------------------------------------------------------------------------------------
class _Env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from distributed_amd.parallel import runtime

        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)
        runtime.shutdown()
        tf.keras.backend.clear_session()

    def __exit__(self, *a):
        from distributed_amd.parallel import runtime

        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        runtime.shutdown()


NATIVE = dict(DAMD_NATIVE_GRAPH="1", DAMD_FUSED="0", DAMD_STRICT_NATIVE="1")


def _prefix(size, pad):
    return [L.ZeroPadding2D(pad, input_shape=(size, size, 3)), L.RandomCrop(size, size), L.RandomFlip("horizontal")]


def _net(prefix, size=16, stride=1):
    """A tiny conv net; ``prefix``: input layers ahead of it (None: the net alone on
    size x size x 3).  stride 2 makes the first conv a packed-tap stem (4-channel input)."""
    kw = {} if prefix else {"input_shape": (size, size, 3)}
    m = tf.keras.Sequential(list(prefix or []) + [
        L.Conv2D(8, 3, strides=stride, padding="same", activation="relu", **kw), L.MaxPooling2D(2), L.Flatten(),
        L.Dense(10)])
    m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
              optimizer=tf.keras.optimizers.SGD(learning_rate=0.05, momentum=0.9), metrics=["accuracy"])
    return m


def _data(n, size, seed=0):
    # k / 128, k < 256: exact in bf16, so the device batch is the host batch
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 256, (n, size, size, 3)) / 128.0).astype(np.float32), rng.integers(0, 10, n)


def _randomize(m, seed):
    rng = np.random.default_rng(seed)
    m.set_weights([rng.normal(0, 0.1, v.shape).astype(np.float32) for v in m.get_weights()])
    return m.get_weights()


class _Grab(tf.keras.callbacks.Callback):
    """After every step: the engine's gathered batch and its augmentation node's output."""

    needs_batch_hooks = True

    def __init__(self):
        super().__init__()
        self.x0, self.aug = [], []

    def on_train_batch_end(self, batch, logs=None):
        e = self.model._engine
        e.sync()
        assert e.nodes[0].kind == "Augment"
        self.x0.append(e.x0.buf.float().cpu().numpy())
        self.aug.append(e.nodes[0].out.buf.float().cpu().numpy())


def test_fresh_draws_every_step_eager_and_replayed():
    x8, y8 = _data(8, 16)
    x, y = np.tile(x8, (3, 1, 1, 1)), np.tile(y8, 3)  # the same 8 rows at steps 1, 2, 3
    with _Env(DAMD_GRAPH="0", **NATIVE):
        m = _net(_prefix(16, 2))
        w0 = _randomize(m, 1)
        grab = _Grab()
        m.fit(x, y, batch_size=8, epochs=1, shuffle=False, verbose=0, callbacks=[grab])
        assert m._engine.name == "native_graph" and not m._engine.use_graph
        stages = m._engine.nodes[0].attrs["stages"]
        assert stages == H.aug_stages(m.layers[:3], L.augment_seeds(m), 16, 16)[0]
        we = m.get_weights()
    assert len(grab.aug) == 3
    for t in (1, 2, 3):
        x0 = grab.x0[t - 1]
        assert np.array_equal(x0[..., :3], x8) and not x0[..., 3:].any()
        assert np.array_equal(grab.aug[t - 1], H.augment_reference(x0, stages, t, 0, True)), t
    assert not any(np.array_equal(grab.aug[a], grab.aug[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    with _Env(DAMD_GRAPH="1", **NATIVE):
        m = _net(_prefix(16, 2))
        m.set_weights(w0)
        m.fit(x, y, batch_size=8, epochs=1, shuffle=False, verbose=0)
        assert m._engine.name == "native_graph" and m._engine.graph is not None
        wg = m.get_weights()
    assert all(np.array_equal(a, b) for a, b in zip(we, wg))
    assert not all(np.array_equal(a, b) for a, b in zip(we, w0))


@pytest.mark.parametrize("n", [16, 12])  # 12: a short final batch
@pytest.mark.parametrize("stride", [1, 2])  # 2: the packed-tap stem, 4-channel pixels
def test_training_equals_training_on_oracle_augmented_data(n, stride):
    x, y = _data(n, 16, seed=3)
    with _Env(**NATIVE):
        a = _net(_prefix(16, 2), stride=stride)
        w0 = _randomize(a, 2)
        ha = a.fit(x, y, batch_size=8, epochs=1, shuffle=False, verbose=0)
        assert a._engine.name == "native_graph" and a._engine.cin_pad == (4 if stride == 2 else 8)
        stages = a._engine.nodes[0].attrs["stages"]
        wa = a.get_weights()
    xa = np.concatenate([H.augment_reference(x[:8], stages, 1, 0, True), H.augment_reference(x[8:], stages, 2, 0, True)])
    assert xa.shape == x.shape and not np.array_equal(xa, x)
    with _Env(**NATIVE):
        b = _net(None, stride=stride)
        b.set_weights(w0)
        hb = b.fit(xa, y, batch_size=8, epochs=1, shuffle=False, verbose=0)
        assert b._engine.name == "native_graph" and not any(nd.kind == "Augment" for nd in b._engine.nodes)
        wb = b.get_weights()
    assert all(np.array_equal(p, q) for p, q in zip(wa, wb))
    assert ha.history == hb.history
    assert not all(np.array_equal(p, q) for p, q in zip(wa, w0))


def test_native_inference_centres_the_crop():
    x, y = _data(21, 16, seed=5)  # batch 8: a short final batch
    with _Env(DAMD_NATIVE_INFER="1", DAMD_STRICT_NATIVE="1"):
        a = _net([L.RandomCrop(12, 12, input_shape=(16, 16, 3)), L.RandomFlip()], size=12)
        b = _net(None, size=12)
        a.set_weights(_randomize(b, 6))
        pa, pb = a.predict(x, batch_size=8), b.predict(x[:, 2:14, 2:14], batch_size=8)
        ea = a.evaluate(x, y, batch_size=8, verbose=0)
        eb = b.evaluate(x[:, 2:14, 2:14], y, batch_size=8, verbose=0)
        plans = a.__dict__.get("_infer_plans", {})
        assert plans and all(p.nodes[0].kind == "Augment" and p.name == "native_infer" for p in plans.values())
    assert pa.shape == (21, 10) and np.array_equal(pa, pb)
    assert ea == eb


def test_strict_native_training_with_validation():
    x, y = _data(24, 16, seed=7)
    records = []

    class _Keep(logging.Handler):
        def emit(self, r):
            records.append(r)

    from distributed_amd.utils import logging as dlog

    h = _Keep(level=logging.WARNING)
    dlog.get_logger().addHandler(h)
    try:
        with _Env(DAMD_NATIVE_INFER="1", **NATIVE):
            m = _net(_prefix(16, 2))
            hist = m.fit(x[:16], y[:16], batch_size=8, epochs=2, shuffle=True, verbose=0,
                         validation_data=(x[16:], y[16:]))
            assert m._engine.name == "native_graph"
            assert int(m.optimizer.iterations) == 4
    finally:
        dlog.get_logger().removeHandler(h)
    assert np.isfinite(hist.history["loss"]).all() and np.isfinite(hist.history["val_loss"]).all()
    assert not [r.getMessage() for r in records if "PyTorch" in r.getMessage() or "fallback" in r.getMessage()]
