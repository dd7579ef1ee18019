"""The flagship forward kernel's wave mapping (fwd_flag, convnet_step2.hip: conv tiles, the
pooled / code stores and the dense-1 hand-off spread over the block's waves) against the
generic forward of the same build (DAMD_SPECIALISED=0), which keeps the plain mapping on 512
threads: the forward's own outputs and the weights are the same bits.

B = 64 (the only batch the specialised kernels take) on a few hundred synthetic rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FEAT, HID, NF, B = 5408, 64, 32, 64
NPOS = FEAT // NF  # 169 pooled positions; the fwd slices hold 3: slice 56 holds position 168 only


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


def _arms(monkeypatch, u8, momentum, nesterov, graph):
    """Per arm (specialised, generic): the forward's outputs after step 1 -- read before the
    flush, with the argmax codes pre-filled with 0xFF -- and the weights after 1 and 3 steps.
    Computed once per configuration and shared by the tests below."""
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
        eng.code.fill_(0xFF)
        torch.cuda.synchronize()
        if graph:
            eng.prepare(1)
        eng.run(1)
        eng.trainer.sync(0.0)  # (no flush: bwd has not yet zeroed this step's dense-1 parity)
        if graph:
            assert eng.trainer.num_graphs >= 1
        r = {"pooled": eng.pooled.view(torch.int16).cpu().numpy().copy(),
             "code": eng.code.cpu().numpy().copy(),
             "hacc": eng.hacc.cpu().numpy().copy(),
             "threads": (eng.trainer.fwd_threads, eng.trainer.fwd_compiled_threads)}
        eng.sync()
        r["w1"] = [w.copy() for w in m.get_weights()]
        eng.run(2)
        eng.finish()
        r["w3"] = [w.copy() for w in m.get_weights()]
        out.append(r)
    _CACHE[key] = out
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, True)], ids=["sgd", "nesterov"])
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "fp32"])
def test_forward_outputs_and_weights_bitwise(u8, momentum, nesterov, graph, monkeypatch):
    """After step 1 the pooled tile, the argmax codes and the live parity of the dense-1
    fixed-point sums; after 1 and 3 steps every weight: specialised == generic, bit for bit."""
    _need_gpu()
    s, g = _arms(monkeypatch, u8, momentum, nesterov, graph)
    assert np.array_equal(s["pooled"], g["pooled"])
    assert np.array_equal(s["code"], g["code"])
    # step 1 runs on parity 0: hacc[0] holds its sums (64 rows x 64 int64), hacc[1] is clear
    live = s["hacc"][:B * HID]
    assert np.count_nonzero(live) > B * HID // 2, np.count_nonzero(live)
    assert np.array_equal(s["hacc"], g["hacc"])
    assert np.count_nonzero(s["pooled"]) > 0 and s["code"].max() <= 7  # every code was written
    for k in ("w1", "w3"):
        for a, b in zip(s[k], g[k]):
            assert a.dtype == b.dtype and np.array_equal(a, b), k
    assert any(np.abs(a - b).max() > 0 for a, b in zip(s["w1"], s["w3"]))  # steps 2, 3 moved them


def test_short_last_slice(monkeypatch):
    """Slice 56 holds one position (168) where the block's tiles have room for three.  Its
    pooled values and codes are written and equal the generic kernel's; the two positions
    past it (169, 170) are not stored: in the [image][5408] code buffer they would land on
    positions 0 and 1 of the next image, so every code byte is a valid code (none of the
    0xFF pre-fill left, none doubled) that agrees with its pooled value -- a code of the
    unstaged rows does not -- and the bytes there equal the generic kernel's."""
    _need_gpu()
    s, g = _arms(monkeypatch, True, 0.0, False, False)
    code, pooled = s["code"], s["pooled"].reshape(FEAT, -1)[:, :B]  # [b][k] / [k][b]
    last = slice((NPOS - 1) * NF, FEAT)
    assert np.array_equal(code[:, last], g["code"][:, last])
    assert np.array_equal(pooled[last], g["pooled"].reshape(FEAT, -1)[last, :B])
    assert np.count_nonzero(pooled[last]) > 0  # position 168 was computed, not zero-filled
    assert code.max() <= 7 and (code[:, last] <= 7).all()
    # bit 2 of a code: the pooled value is > 0 (bf16 bits > 0 as int16: positive, non-zero)
    assert np.array_equal((code & 4) != 0, pooled.T > 0)
    # where positions 169 / 170 of image b would land: image b + 1, positions 0 and 1
    assert np.array_equal(code[1:, :2 * NF], g["code"][1:, :2 * NF])


def test_launch_dimension_matches_compiled_thread_count(monkeypatch):
    """The threads per block the engine launches the specialised forward with are the ones
    the kernel was compiled for (its launch bound); the generic forward stays on 512."""
    _need_gpu()
    s, g = _arms(monkeypatch, True, 0.0, False, False)
    assert s["threads"][0] == s["threads"][1], s["threads"]
    assert g["threads"] == (512, 512), g["threads"]
