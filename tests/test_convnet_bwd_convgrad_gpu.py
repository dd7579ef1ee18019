"""The flagship backward's conv gradient on pre-decoded codes (CfgFlagBwd::CGPRE in
csrc/kernels/convnet_step2.hip: the staging waves translate each argmax code into an offset
byte and a mask byte, the gradient reads entries, dP values and x taps in two LDS batches and
does not skip the short last slice's second position) against the generic kernels of the same
build (DAMD_SPECIALISED=0), which keep conv_grad as it was.  Bit for bit: the 320 int64
conv-gradient sums of the step's hconv parity, and the conv weights after the next forward has
applied them.

The flagship kernel has one size -- 64 images, 85 slices of 2 pooled positions, the last of
one -- so that is the shape.  Inputs: random rows; conv parameters that make every
pre-activation negative (every code `off`: the sums are exactly 0); a batch whose only non-zero
pixels feed pooled position 168, the short last slice; each with uint8 and fp32 rows.  One case
fills every CU's LDS with NaNs (diag.hip) ahead of each step: a read of a row nobody staged
-- the last slice's second position has none -- would poison the sums."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, NCONV, NF = 64, 320, 32
POISON_BLOCKS = 1024


def _x(kind, u8, n=2 * B):
    rng = np.random.default_rng(31)
    if u8:  # exactly k / 255: kept as uint8 rows on the device
        x = rng.integers(1, 256, (n, 28, 28, 1)).astype(np.uint8) / 255.0
    else:
        x = rng.random((n, 28, 28, 1), dtype=np.float32) + np.float32(0.01)
    if kind == "pos168":
        # pooled position 168 = (12, 12) pools conv outputs (24..25, 24..25): pixels 24..27; pixels
        # 26..27 of both axes reach no other position
        keep = np.zeros_like(x)
        keep[:, 26:28, 26:28] = x[:, 26:28, 26:28]
        x = keep
    return x, rng.integers(0, 10, n).astype(np.int64)


def _poison():
    from distributed_amd.native import require_C

    torch.cuda.synchronize()
    require_C().lds_poison(POISON_BLOCKS, 0)
    torch.cuda.synchronize()


_CACHE = {}


def _two_steps(monkeypatch, spec, kind, u8, poison=False):
    """Two eager steps; returns the hconv sums of step 1's parity right after step 1, the conv
    kernel and bias before the steps and after step 2 (whose forward applied step 1's gradient)
    and the raw codes of step 1.  Computed once per configuration."""
    key = (spec, kind, u8, poison)
    if key in _CACHE:
        return _CACHE[key]
    import distributed_amd as tf

    monkeypatch.setenv("DAMD_SPECIALISED", "1" if spec else "0")
    monkeypatch.setenv("DAMD_X_U8", "1" if u8 else "0")
    monkeypatch.setenv("DAMD_GRAPH", "0")
    tf.set_seed(9)
    m = tf.models.mnist_cnn()
    m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
              optimizer=tf.keras.optimizers.SGD(learning_rate=0.05, momentum=0.9, nesterov=True),
              metrics=["accuracy"])
    w = [a.copy() for a in m.get_weights()]
    assert w[0].shape == (3, 3, 1, NF) and w[1].shape == (NF,)
    if kind == "alloff":  # x > 0, weights < 0, bias < 0: every conv pre-activation is negative
        w[0] = -np.abs(w[0]) - np.float32(0.01)
        w[1] = np.full_like(w[1], -0.5)
        m.set_weights(w)
    x, y = _x(kind, u8)
    eng = m._get_engine(B, B)
    assert eng.name == "fused_convnet"
    assert eng.step_kernels == ("specialised" if spec else "generic")
    eng.bind(x, y)
    assert eng.feed.x_u8 == u8
    eng.start_epoch(0, shuffle=False)
    eng.trainer.sync(0.0)
    assert eng.trainer.parity == 0
    if poison:
        _poison()
    eng.run(1)
    eng.trainer.sync(0.0)  # (no flush: the step's hconv parity holds its sums)
    r = {"hconv": eng.hconv.cpu().numpy().copy().reshape(-1)[:NCONV], "code": eng.code.cpu().numpy().copy(),
         "before": w[:2]}
    if poison:
        _poison()
    eng.run(1)
    eng.finish()
    r["after"] = [a.copy() for a in m.get_weights()[:2]]
    _CACHE[key] = r
    return r


def _same_as_generic(s, g):
    assert s["hconv"].dtype == np.int64 and s["hconv"].shape == (NCONV,)
    assert np.array_equal(s["code"], g["code"])
    assert np.array_equal(s["hconv"], g["hconv"]), np.flatnonzero(s["hconv"] != g["hconv"])[:8]
    for a, b in zip(s["after"], g["after"]):
        assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
        assert np.isfinite(a).all()


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "fp32"])
@pytest.mark.parametrize("kind", ["random", "alloff", "pos168"])
def test_conv_gradient_equals_generic_bitwise(kind, u8, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    s = _two_steps(monkeypatch, True, kind, u8)
    g = _two_steps(monkeypatch, False, kind, u8)
    _same_as_generic(s, g)
    on = (s["code"].reshape(B, -1, NF) & 4) != 0  # [image][position][channel]
    if kind == "alloff":
        assert not on.any()
        assert not s["hconv"].any()  # exactly 0: every product had d = +0
        for a, b in zip(s["after"], s["before"]):
            assert np.array_equal(a, b)  # a zero gradient, no velocity: the parameters stay
    else:
        if kind == "pos168":
            # (most taps of the one live window see only zero pixels: some sums are 0 by data)
            assert on[:, 168].any() and not on[:, :168].any()
            assert s["hconv"][:288].any() and s["hconv"][288:].any()  # weight taps, bias sums
        else:
            assert on[:, 168].any() and on[:, :168].any()
            assert np.count_nonzero(s["hconv"]) > NCONV // 2
        assert any(not np.array_equal(a, b) for a, b in zip(s["after"], s["before"]))


def test_conv_gradient_ignores_stale_lds(monkeypatch):
    """NaNs in every CU's LDS ahead of each step (the backward's LDS is larger than the forward's,
    and more CUs than the forward has blocks: the conv role's staged rows lie in words the forward
    never wrote): the sums and weights of the unpoisoned run."""
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    clean = _two_steps(monkeypatch, True, "random", True)
    dirty = _two_steps(monkeypatch, True, "random", True, poison=True)
    _same_as_generic(dirty, clean)
    last = _two_steps(monkeypatch, True, "pos168", True, poison=True)
    _same_as_generic(last, _two_steps(monkeypatch, True, "pos168", True))
