"""The forward step kernels never read an LDS word nobody staged: with every CU's LDS filled
with a NaN pattern (0x7FC07FC0: NaN as fp32 and as two bf16; csrc/kernels/diag.hip) before
each eager step, two steps give the forward outputs and weights of the unpoisoned run, bit for
bit, in both instantiations (specialised, generic) and with uint8 and fp32 rows.  The short
last slice is the case in point: its tiles cover positions whose rows are never staged.

Limit: the backward runs after the forward and sees what the forward left in LDS, not the
poison.  Skips where LDS contents do not survive from one kernel to the next."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, BLOCKS = 64, 1024  # poison blocks: one per CU at a time, several rounds over every CU


def _poison():
    from distributed_amd.native import require_C

    torch.cuda.synchronize()
    require_C().lds_poison(BLOCKS, 0)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def lds_retained():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from distributed_amd.native import require_C

    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    _poison()
    require_C().lds_count(BLOCKS, n.data_ptr(), 0)
    torch.cuda.synchronize()
    found = int(n.item())
    print("poison words found in unwritten LDS:", found)
    if found == 0:
        pytest.skip("LDS contents are not retained between kernels on this device: nothing to poison")
    return found


def _run(monkeypatch, u8, spec, poison):
    import distributed_amd as tf

    monkeypatch.setenv("DAMD_X_U8", "1" if u8 else "0")
    monkeypatch.setenv("DAMD_GRAPH", "0")
    monkeypatch.setenv("DAMD_SPECIALISED", "1" if spec else "0")
    tf.set_seed(5)
    m = tf.models.mnist_cnn()
    m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
              optimizer=tf.keras.optimizers.SGD(learning_rate=0.05, momentum=0.9, nesterov=True),
              metrics=["accuracy"])
    rng = np.random.default_rng(23)
    if u8:
        x = rng.integers(0, 256, (2 * B, 28, 28, 1)).astype(np.uint8) / 255.0
    else:
        x = rng.random((2 * B, 28, 28, 1), dtype=np.float32)
    y = rng.integers(0, 10, 2 * B).astype(np.int64)
    eng = m._get_engine(B, B)
    assert eng.name == "fused_convnet"
    assert eng.step_kernels == ("specialised" if spec else "generic")
    eng.bind(x, y)
    assert eng.feed.x_u8 == u8
    eng.start_epoch(0, shuffle=False)
    eng.trainer.sync(0.0)
    out = []
    for _ in range(2):
        if poison:
            _poison()
        eng.run(1)
        eng.trainer.sync(0.0)  # (no flush yet: the live dense-1 parity still holds the forward's sums)
        r = {"pooled": eng.pooled.view(torch.int16).cpu().numpy().copy(), "code": eng.code.cpu().numpy().copy(),
             "hacc": eng.hacc.cpu().numpy().copy()}
        eng.sync()
        r["weights"] = [w.copy() for w in m.get_weights()]
        out.append(r)
    met = eng.end_epoch()
    eng.finish()
    return out, met


@pytest.mark.parametrize("spec", [True, False], ids=["specialised", "generic"])
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "fp32"])
def test_forward_ignores_stale_lds(u8, spec, lds_retained, monkeypatch):
    clean, mc = _run(monkeypatch, u8, spec, poison=False)
    dirty, md = _run(monkeypatch, u8, spec, poison=True)
    for step, (a, b) in enumerate(zip(clean, dirty), 1):
        for k in ("pooled", "code", "hacc"):
            assert np.array_equal(a[k], b[k]), (step, k)
        for i, (wa, wb) in enumerate(zip(a["weights"], b["weights"])):
            assert np.array_equal(wa, wb), (step, i)
            assert np.isfinite(wb).all(), (step, i)
    assert mc == md and np.isfinite(md["loss"]), (mc, md)
    assert any(np.abs(x - y).max() > 0 for x, y in zip(clean[0]["weights"], clean[1]["weights"]))  # step 2 trained
