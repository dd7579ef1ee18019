"""The flagship backward with a role per block (bwd_flag, CfgFlagBwd::SPLIT in convnet_step2.hip:
2 x 85 blocks -- the conv role of a slice runs dP, the conv gradient and the hconv atomics, its
W1 role the dW1 MFMAs, the eager update and everything off the chain) and the bf16 copy of W1
with one buffer per step parity, which the roles need: the conv block of a slice reads the
bf16 slice its W1 block rewrites, and the two are not ordered.

The yardstick is the generic backward of the same build (DAMD_SPECIALISED=0): one block per
slice on 512 threads.  Every comparison is bit for bit.

The flagship configuration has one size -- 64 images, 169 pooled positions, 85 bwd slices, the
last of one position -- so the shapes are fixed; a step takes microseconds."""
import shutil
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]

FEAT, HID, NF, B = 5408, 64, 32, 64
NPOS = FEAT // NF
NS_BWD = (NPOS + 1) // 2  # 85 slices of 2 positions, the last holds position 168 only
NCONV = 320
HACC_FILL = 0x0123456789ABCDEF
BF16_NAN = 0x7FC1  # a quiet NaN pattern (as int16 bits)

# everything a step writes or leaves behind, read raw (no flush) after each step
_STATE = ("G", "hconv", "P", "V", "calt", "w1bf", "w1bf2", "xnext", "xtag", "hacc")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _model(momentum, nesterov, seed=21):
    import distributed_amd as tf

    tf.set_seed(seed)
    m = tf.models.mnist_cnn()
    m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
              optimizer=tf.keras.optimizers.SGD(learning_rate=0.05, momentum=momentum, nesterov=nesterov),
              metrics=["accuracy"])
    return m


def _data(u8, n=B * 6):
    rng = np.random.default_rng(17)
    if u8:  # exactly k / 255: kept as uint8 rows on the device
        x = rng.integers(0, 256, (n, 28, 28, 1)).astype(np.uint8) / 255.0
    else:
        x = rng.random((n, 28, 28, 1), dtype=np.float32)
    return x, rng.integers(0, 10, n).astype(np.int64)


def _np(t):
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy().copy()


def _snap(eng):
    eng.trainer.sync(0.0)  # (no flush: the step parity stays what the steps left)
    r = {k: _np(getattr(eng, k)) for k in _STATE if k != "w1bf2"}
    r["w1bf2"] = np.stack([_np(b) for b in eng.w1bf_bufs])  # both parity buffers of the bf16 copy
    return r


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _weights_same(wa, wb, what=""):
    for a, b in zip(wa, wb):
        assert a.dtype == b.dtype and np.array_equal(a, b), what


def _engine(monkeypatch, spec, u8, momentum, nesterov, graph=False, graph_steps=1):
    monkeypatch.setenv("DAMD_SPECIALISED", "1" if spec else "0")
    monkeypatch.setenv("DAMD_X_U8", "1" if u8 else "0")
    monkeypatch.setenv("DAMD_GRAPH", "1" if graph else "0")
    monkeypatch.setenv("DAMD_GRAPH_STEPS", str(graph_steps))
    m = _model(momentum, nesterov)
    eng = m._get_engine(B, B)
    assert eng.name == "fused_convnet"
    assert eng.step_kernels == ("specialised" if spec else "generic")
    x, y = _data(u8)
    eng.bind(x, y)
    assert eng.feed.x_u8 == u8
    eng.start_epoch(0, shuffle=False)
    eng.trainer.sync(0.0)
    return m, eng


_CACHE = {}


def _four_steps(monkeypatch, spec, u8, momentum, nesterov, poison=False):
    """4 eager steps (parities 0, 1, 0, 1: both bf16 buffers are read and written twice).
    Before each step the dead parity of the dense-1 sums is filled with a non-zero pattern
    and, with ``poison``, the bf16 W1 buffer that is not live with NaNs.  Returns the raw state
    after each step (no flush in between) and the weights after the last.  Computed once per
    configuration and shared by the tests below; nothing changes it afterwards."""
    key = (spec, u8, momentum, nesterov, poison)
    if key in _CACHE:
        return _CACHE[key]
    m, eng = _engine(monkeypatch, spec, u8, momentum, nesterov)
    half = eng.hacc.numel() // 2
    r = {"steps": [], "blocks": eng.trainer.bwd_blocks, "written_nan": []}
    for k in range(4):
        par = eng.trainer.parity
        assert par == (k & 1)
        (eng.hacc[half:] if par == 0 else eng.hacc[:half]).fill_(HACC_FILL)
        if poison:
            eng.w1bf_bufs[par ^ 1].view(torch.int16).fill_(BF16_NAN)
        torch.cuda.synchronize()
        eng.run(1)
        s = _snap(eng)
        assert eng.trainer.parity == par ^ 1
        # the buffer this step wrote is the one the next step reads: `w1bf`, the live one
        assert np.array_equal(s["w1bf"], s["w1bf2"][par ^ 1])
        r["written_nan"].append(int(np.isnan(eng.w1bf_bufs[par ^ 1].float().cpu().numpy()).sum()))
        r["steps"].append(s)
    eng.finish()
    r["weights"] = [w.copy() for w in m.get_weights()]
    _CACHE[key] = r
    return r


# ---- 1. split against the generic kernels, bit for bit -----------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, False), (0.9, True)],
                         ids=["sgd", "momentum", "nesterov"])
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "fp32"])
def test_roles_equal_generic_bitwise(u8, momentum, nesterov, monkeypatch):
    """After each of 4 consecutive steps everything the backward writes -- the small gradients
    and the metric tail, the hconv sums, the W1 masters and velocities, both bf16 buffers and
    which of them is live, the next-batch staging and its tag, the zeroed dead parity of the
    dense-1 sums -- and the parameters as they stand (masters, conv double buffer) are the
    generic kernels'; so are the weights after the last step."""
    _need_gpu()
    import distributed_amd.native as native

    C = native.load_C()
    s = _four_steps(monkeypatch, True, u8, momentum, nesterov)
    g = _four_steps(monkeypatch, False, u8, momentum, nesterov)
    assert g["blocks"] == NS_BWD
    assert s["blocks"] == (2 * NS_BWD if C.convnet2_bwd_flag_split() else NS_BWD)
    for k in range(4):
        _same(s["steps"][k], g["steps"][k], f"step {k + 1}")
        st, par = s["steps"][k], k & 1
        half = st["hacc"].size // 2
        dead = st["hacc"][half:] if par == 0 else st["hacc"][:half]
        live = st["hacc"][:half] if par == 0 else st["hacc"][half:]
        assert not dead.any() and np.count_nonzero(live) > B * HID // 2
        assert np.count_nonzero(st["hconv"][par * NCONV:(par + 1) * NCONV]) > NCONV // 2
        assert np.count_nonzero(st["xnext"]) > 0 and st["xtag"][0] != 0
        # the eager update wrote the other buffer, all of it; the one it read is untouched
        assert np.count_nonzero(st["w1bf2"][par ^ 1] != st["w1bf2"][par]) > FEAT * HID // 4
        if k:
            assert np.array_equal(st["w1bf2"][par], s["steps"][k - 1]["w1bf2"][par])
            assert np.count_nonzero(_bits(st["P"]) != _bits(s["steps"][k - 1]["P"])) > FEAT * HID // 4
    _weights_same(s["weights"], g["weights"])


# ---- 2. the readers read only the live buffer ----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("spec", [True, False], ids=["roles", "generic"])
def test_readers_read_only_the_live_bf16_buffer(spec, monkeypatch):
    """The bf16 W1 buffer that is not live filled with NaNs before every step, at both
    parities: every output and weight equals the unpoisoned run's (no reader touched it), and
    after the step the buffer is the complete new copy -- no NaN left, the last slice's single
    position included."""
    _need_gpu()
    clean = _four_steps(monkeypatch, spec, True, 0.9, True)
    dirty = _four_steps(monkeypatch, spec, True, 0.9, True, poison=True)
    assert dirty["written_nan"] == [0, 0, 0, 0], dirty["written_nan"]
    for k in range(4):
        _same(clean["steps"][k], dirty["steps"][k], f"step {k + 1}")
        last = dirty["steps"][k]["w1bf2"][(k & 1) ^ 1][(NPOS - 1) * NF * HID:]
        assert last.size == NF * HID and not (last == BF16_NAN).any()
        assert np.isfinite(dirty["steps"][k]["G"]).all()
    _weights_same(clean["weights"], dirty["weights"])


# ---- 3. flagship <-> generic transitions -----------------------------------------------------
def _transitions(monkeypatch, spec, reload_weights):
    """3 flagship steps (the parity ends odd), one step at 32 images -- a batch
    convnet2_specialised rejects, so a generic launch whatever the switch --, 3 flagship steps
    again; with ``reload_weights`` a set_weights of perturbed values in the middle of each
    flagship stretch.  Returns the weights after every stage."""
    monkeypatch.setenv("DAMD_SPECIALISED", "1" if spec else "0")
    monkeypatch.setenv("DAMD_X_U8", "1")
    monkeypatch.setenv("DAMD_GRAPH", "0")
    m = _model(0.9, True, seed=5)
    x, y = _data(True)
    out, kernels = [], []
    for stage, bsz in enumerate((B, 32, B)):
        eng = m._get_engine(bsz, bsz)
        assert eng.name == "fused_convnet"
        kernels.append(eng.step_kernels)
        eng.bind(x, y)
        eng.start_epoch(stage, shuffle=False)
        if bsz == B:
            eng.run(1)
            if reload_weights:  # (get_weights applies what is pending; set_weights re-derives the copy)
                w = [a + np.float32(2.0 ** -7) * np.sign(a) for a in m.get_weights()]
                m.set_weights(w)
            eng.run(2)
            eng.trainer.sync(0.0)
            assert eng.trainer.parity == (0 if reload_weights else 1)
        else:
            eng.run(1)
        out.append([a.copy() for a in m.get_weights()])
    assert kernels == (["specialised", "generic", "specialised"] if spec else ["generic"] * 3), kernels
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("reload_weights", [False, True], ids=["steps", "set_weights"])
def test_flagship_generic_transitions_bitwise(reload_weights, monkeypatch):
    _need_gpu()
    s = _transitions(monkeypatch, True, reload_weights)
    g = _transitions(monkeypatch, False, reload_weights)
    for k, (a, b) in enumerate(zip(s, g)):
        _weights_same(a, b, f"stage {k}")
    assert any(np.abs(a - b).max() > 0 for a, b in zip(s[0], s[2]))


@pytest.mark.gpu
def test_checkpoint_reload_between_steps_bitwise(monkeypatch, tmp_path):
    """save_weights after an odd number of steps, two more steps, load_weights, two steps:
    the reloaded bf16 copy is the one the next forward reads, at either parity."""
    _need_gpu()
    res = []
    for spec in (True, False):
        m, eng = _engine(monkeypatch, spec, True, 0.9, False)
        eng.run(3)
        path = str(tmp_path / f"w{int(spec)}.weights.h5")
        m.save_weights(path)
        eng.run(1)
        m.load_weights(path)
        eng.run(2)
        eng.finish()
        res.append([a.copy() for a in m.get_weights()])
    _weights_same(res[0], res[1])


# ---- 4. replay equals eager --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("graph_steps", [4, 1], ids=["one-4-step-graph", "both-parities-graphs"])
def test_graph_replay_equals_eager_launches(graph_steps, monkeypatch):
    """4 steps replayed from captured graphs -- one 4-step graph, or the 1-step graphs of both
    parities alternating -- against 4 eager launches: the same raw state and weights."""
    _need_gpu()
    eager = _four_steps(monkeypatch, True, True, 0.9, True)
    m, eng = _engine(monkeypatch, True, True, 0.9, True, graph=True, graph_steps=graph_steps)
    # (the eager arm pre-fills the dead parity of the dense-1 sums before each step; every
    # step zeroes it again, so the state after 4 steps does not depend on that)
    eng.prepare(4)
    eng.run(4)
    s = _snap(eng)
    assert eng.trainer.num_graphs >= (2 if graph_steps == 1 else 1)
    _same(s, eager["steps"][3])
    eng.finish()
    _weights_same([w.copy() for w in m.get_weights()], eager["weights"])


# ---- 5. launch contract (no device needed) ---------------------------------------------------
def test_launch_contract():
    """2 x NS blocks with the roles on (NS without), and the LDS of either role -- the launch
    asks for the larger -- within the 160 KB of one workgroup."""
    from distributed_amd import native

    C = native.load_C()
    ns = C.convnet_num_slices(2)
    assert ns == NS_BWD
    assert C.convnet2_bwd_flag_blocks() == (2 * ns if C.convnet2_bwd_flag_split() else ns)
    conv, w1 = C.convnet2_bwd_role_lds_bytes(2, 0), C.convnet2_bwd_role_lds_bytes(2, 1)
    assert 0 < w1 < conv <= 160 * 1024, (conv, w1)
    if C.convnet2_bwd_flag_split():
        assert C.convnet2_bwd_flag_lds_bytes(2) == max(conv, w1)


_HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if Path("/opt/rocm/bin/hipcc").exists() else None)


@pytest.mark.skipif(_HIPCC is None, reason="needs hipcc")
@pytest.mark.timeout(600)
def test_split_switch_off_builds_the_one_block_per_slice_kernel(tmp_path):
    """DAMD_BWD_SPLIT=0 compiles (no spills, no scratch) and its grid is one block per slice:
    the grid constant is checked by the compiler itself, in a host-only pass over the kernel
    file with a static_assert appended; the same assertion fails to compile with the switch on
    (so it does test the switch), where the grid is two blocks per slice."""
    import subprocess

    sys.path.insert(0, str(ROOT / "scripts"))
    import isa_table

    rows, _ = isa_table.table(ROOT / "csrc" / "kernels" / "convnet_step2.hip", defines=("DAMD_BWD_SPLIT=0",))
    for name, k in rows:
        if "bwd_flag" in name:
            assert k["sgpr_spill_count"] == 0 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0

    def grid_is(blocks, split):
        tu = tmp_path / f"grid_{blocks}_{split}.hip"
        tu.write_text('#include "kernels/convnet_step2.hip"\n'
                      f"static_assert(damd::convnet2::CfgFlagBwd::GRID == {blocks}, \"grid\");\n")
        r = subprocess.run([_HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-fsyntax-only", "-std=c++17",
                            f"-DDAMD_BWD_SPLIT={split}", "-I", str(ROOT / "csrc"), "-I", str(ROOT / "csrc" / "include"),
                            "-I", str(ROOT / "csrc" / "runtime"), str(tu)], capture_output=True, text=True)
        return r.returncode == 0

    assert grid_is(NS_BWD, 0)
    assert grid_is(2 * NS_BWD, 1)
    assert not grid_is(NS_BWD, 1)
