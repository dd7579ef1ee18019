"""The flagship backward kernel's wave mapping (bwd_flag, convnet_step2.hip: h, body staging,
dh / dW1 / dP tiles and the conv gradient's taps spread over the block's waves, dps in an LDS
region of its own, the dead-parity zeroing and the next-batch store issued early) against the
generic backward of the same build (DAMD_SPECIALISED=0), which keeps the plain mapping on 512
threads: everything the backward writes and the weights are the same bits.

B = 64 (the only batch the specialised kernels take) on 256 synthetic rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FEAT, HID, NF, B = 5408, 64, 32, 64
NPOS = FEAT // NF  # 169 pooled positions; the bwd slices hold 2: slice 84 holds position 168 only
NCONV, NSMALL = 320, 714
OFF_W1 = NCONV
OFF_B1 = OFF_W1 + FEAT * HID
NPARAM = OFF_B1 + NSMALL
HACC_FILL = 0x0123456789ABCDEF


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _model(momentum, nesterov):
    import distributed_amd as tf

    tf.set_seed(21)
    m = tf.models.mnist_cnn()
    m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
              optimizer=tf.keras.optimizers.SGD(learning_rate=0.05, momentum=momentum, nesterov=nesterov),
              metrics=["accuracy"])
    return m


def _data(u8):
    rng = np.random.default_rng(17)
    if u8:  # exactly k / 255: kept as uint8 rows on the device
        x = rng.integers(0, 256, (B * 4, 28, 28, 1)).astype(np.uint8) / 255.0
    else:
        x = rng.random((B * 4, 28, 28, 1), dtype=np.float32)
    return x, rng.integers(0, 10, B * 4).astype(np.int64)


_CACHE = {}
_BWD_WRITES = ("G", "hconv", "P", "V", "w1bf", "xnext", "xtag", "hacc")


def _arms(monkeypatch, u8, momentum, nesterov, graph):
    """Per arm (specialised, generic): what the backward writes, read after step 1 before any
    flush -- the dead parity of the dense-1 sums pre-filled with a non-zero pattern, the
    parameters also read before the step -- and the weights after 1 and 3 steps.  Computed
    once per configuration and shared by the tests below."""
    key = (u8, momentum, nesterov, graph)
    if key in _CACHE:
        return _CACHE[key]
    monkeypatch.setenv("DAMD_X_U8", "1" if u8 else "0")
    monkeypatch.setenv("DAMD_GRAPH", "1" if graph else "0")
    monkeypatch.setenv("DAMD_GRAPH_STEPS", "1")
    x, y = _data(u8)
    out = []
    for spec in ("1", "0"):
        monkeypatch.setenv("DAMD_SPECIALISED", spec)
        m = _model(momentum, nesterov)
        eng = m._get_engine(B, B)
        assert eng.name == "fused_convnet"
        assert eng.step_kernels == ("specialised" if spec == "1" else "generic")
        eng.bind(x, y)
        assert eng.feed.x_u8 == u8
        eng.start_epoch(0, shuffle=False)
        eng.trainer.sync(0.0)
        # step 1 runs on parity 0: its backward zeroes parity 1 (nothing reads it before that)
        half = eng.hacc.numel() // 2
        eng.hacc[half:].fill_(HACC_FILL)
        torch.cuda.synchronize()
        r = {"P0": eng.P.cpu().numpy().copy()}
        if graph:
            eng.prepare(1)
        eng.run(1)
        eng.trainer.sync(0.0)  # (no flush)
        if graph:
            assert eng.trainer.num_graphs >= 1
        for k in _BWD_WRITES:
            t = getattr(eng, k)
            r[k] = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().copy()
        r["threads"] = (eng.trainer.bwd_threads, eng.trainer.bwd_compiled_threads)
        eng.sync()
        r["w1"] = [w.copy() for w in m.get_weights()]
        eng.run(2)
        eng.finish()
        r["w3"] = [w.copy() for w in m.get_weights()]
        out.append(r)
    _CACHE[key] = out
    return out


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, True)], ids=["sgd", "nesterov"])
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "fp32"])
def test_backward_outputs_and_weights_bitwise(u8, momentum, nesterov, graph, monkeypatch):
    """After step 1, before any flush: the small gradients and the metric tail, the live
    conv-gradient parity, the W1 masters / velocities / bf16 copy, the next-batch staging and
    its tag, the zeroed dead parity of the dense-1 sums; after 1 and 3 steps every weight:
    specialised == generic, bit for bit."""
    _need_gpu()
    s, g = _arms(monkeypatch, u8, momentum, nesterov, graph)
    for k in _BWD_WRITES:
        assert np.array_equal(_bits(s[k]), _bits(g[k])), k
    # small gradients (b1 / W2 / b2) and the metric tail [loss, correct, count]
    small, tail = s["G"][OFF_B1:NPARAM], s["G"][NPARAM:NPARAM + 3]
    assert np.count_nonzero(small) > NSMALL // 2 and np.isfinite(small).all()
    assert tail[0] > 0 and tail[2] == B, tail
    # step 1 adds its conv gradient into parity 0 of hconv
    assert np.count_nonzero(s["hconv"][:NCONV]) > NCONV // 2
    # the eager update moved W1 (master and bf16 copy; the velocity with momentum)
    w1a, w1b = s["P0"][OFF_W1:OFF_B1], s["P"][OFF_W1:OFF_B1]
    assert np.count_nonzero(w1a != w1b) > FEAT * HID // 4
    assert np.count_nonzero(s["w1bf"]) > FEAT * HID // 2
    if momentum:
        assert np.count_nonzero(s["V"][OFF_W1:OFF_B1]) > FEAT * HID // 4
    # the next step's rows were staged and tagged
    assert np.count_nonzero(s["xnext"]) > 0 and s["xtag"][0] != 0
    # the dead parity: every word of the pre-filled pattern zeroed, the live one still holds sums
    half = s["hacc"].size // 2
    assert not s["hacc"][half:].any()
    assert np.count_nonzero(s["hacc"][:half]) > B * HID // 2
    for k in ("w1", "w3"):
        for a, b in zip(s[k], g[k]):
            assert a.dtype == b.dtype and np.array_equal(a, b), k
    assert any(np.abs(a - b).max() > 0 for a, b in zip(s["w1"], s["w3"]))  # steps 2, 3 moved them


def test_short_last_slice(monkeypatch):
    """Slice 84 holds one position (168) where the block's tiles have room for two.  Its W1
    rows are updated and equal the generic kernel's.  Position 169 has no rows: in the flat
    parameter buffer they would land on b1 / W2 / b2 and past the parameters, which no kernel
    of step 1 changes (no update is pending yet) -- they keep their values from before the
    step; the bf16 copy has no slack at all, so its size is the parameter count."""
    _need_gpu()
    s, g = _arms(monkeypatch, True, 0.9, True, False)
    last = slice(OFF_W1 + (NPOS - 1) * NF * HID, OFF_B1)
    for k in ("P", "V"):
        assert np.array_equal(_bits(s[k][last]), _bits(g[k][last])), k
    assert np.count_nonzero(s["P"][last] != s["P0"][last]) > NF * HID // 4  # updated
    assert np.count_nonzero(s["V"][last]) > NF * HID // 4
    assert np.array_equal(s["w1bf"][(NPOS - 1) * NF * HID:], g["w1bf"][(NPOS - 1) * NF * HID:])
    assert np.array_equal(_bits(s["P"][OFF_B1:]), _bits(s["P0"][OFF_B1:]))
    assert np.count_nonzero(s["P0"][OFF_B1 + HID:NPARAM - 10]) > 0  # (W2 is not all zero: a real guard)
    assert np.array_equal(_bits(s["V"][OFF_B1:]), _bits(g["V"][OFF_B1:])) and not s["V"][OFF_B1:].any()
    assert s["w1bf"].size == FEAT * HID and s["P"].size == g["P"].size


def test_launch_dimension_matches_compiled_thread_count(monkeypatch):
    """The threads per block the engine launches the specialised backward with are the ones
    the kernel was compiled for (its launch bound); the generic backward stays on 512."""
    _need_gpu()
    s, g = _arms(monkeypatch, True, 0.9, True, False)
    assert s["threads"][0] == s["threads"][1], s["threads"]
    assert g["threads"] == (512, 512), g["threads"]
