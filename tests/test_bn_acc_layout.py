"""The layout check of the fixed-point BatchNorm accumulators (ops/hip.py acc_reps): every
kernel writes the sticky flag plane behind the last replica, so an accumulator without it
must be refused before any native call.  CPU tensors only: nothing here reaches the device."""
import pytest
import torch

from distributed_amd.ops import hip as H

C = 8


def _bad(words):
    """Tensors that are no accumulator of C channels with ``words`` words per channel."""
    bad = {
        "one replica, no flag plane (1-D)": torch.zeros(words * C, dtype=torch.int64),
        "one row": torch.zeros(1, words * C, dtype=torch.int64),
        "fp32": torch.zeros(2, words * C, dtype=torch.float32),
        "not contiguous": torch.zeros(words * C, 2, dtype=torch.int64).t(),
        "3-D": torch.zeros(2, 1, words * C, dtype=torch.int64),
    }
    if words == 4:
        bad["forward width"] = H.acc_zeros(3, 2 * C, "cpu")
    return bad


@pytest.mark.parametrize("words", [2, 4])
def test_acc_reps_valid_layouts(words):
    for r in (1, 3):
        assert H.acc_reps(H.acc_zeros(r, words * C, "cpu"), C, words) == r
    assert H.acc_reps(torch.zeros(2 * words * C, dtype=torch.int64), C, words) == 1


@pytest.mark.parametrize("words", [2, 4])
def test_acc_reps_refuses(words):
    for what, t in _bad(words).items():
        with pytest.raises(ValueError):
            H.acc_reps(t, C, words)
            pytest.fail(f"accepted: {what}")


def test_acc_reps_refuses_flat_backward_sums():
    """The 1-D [4 C] tensor conv_dgrad's bnred check used to accept (shape[-1] == 4 Cin): the
    kernel's flag write lands past its end."""
    with pytest.raises(ValueError):
        H.acc_reps(torch.zeros(4 * C, dtype=torch.int64), C, 4)


def test_stats_argument_is_checked():
    """The GEMM / split-K finish `stats` argument: fp32 partials pass through, an int64
    accumulator is checked against the column count."""
    assert H._stats_ptrs(None, C) == (0, 0, 1)
    part = torch.zeros(3, 2, C)
    assert H._stats_ptrs(part, C) == (part.data_ptr(), 0, 1)
    acc = H.acc_zeros(3, 4 * C, "cpu")
    assert H._stats_ptrs(acc, C, 4) == (0, acc.data_ptr(), 3)
    for t in _bad(4).values():
        if t.dtype == torch.int64:
            with pytest.raises(ValueError):
                H._stats_ptrs(t, C, 4)
    with pytest.raises(ValueError):
        H._check_stats(torch.zeros(2 * C, dtype=torch.int64), {"stats_T": 1}, C, "conv_fwd")


def test_bnfin_checks_its_accumulator():
    st = torch.zeros(4, C)
    assert H.BNFin(H.acc_zeros(3, 2 * C, "cpu"), None, None, st, None, None, 16, 1e-3, 0.99).args()[1][3] == 3.0
    assert H.BNFin(None, None, None, st, None, None, 16, 1e-3, 0.99).args()[1][3] == 1.0
    for t in _bad(2).values():
        with pytest.raises(ValueError):
            H.BNFin(t, None, None, st, None, None, 16, 1e-3, 0.99)
    with pytest.raises(ValueError):  # a backward accumulator offered as the forward one
        H.BNFin(H.acc_zeros(3, 4 * C, "cpu"), None, None, st, None, None, 16, 1e-3, 0.99)


def test_backward_entry_points_check_before_any_native_call(monkeypatch):
    def no_native():
        raise AssertionError("reached the native module")

    monkeypatch.setattr(H, "_C", no_native)
    x = torch.zeros(2, 4, 4, C, dtype=torch.bfloat16)
    st, co = torch.zeros(4, C), torch.zeros(3, C)
    good = H.acc_zeros(3, 4 * C, "cpu")
    for t in _bad(4).values():
        with pytest.raises(ValueError):
            H.bn_bwd(x, x, 1, x, st, None, co, x, acc=t)
        with pytest.raises(ValueError):
            H.pool_bn_bwd(x, None, x, st, None, co, x, (3, 3), (2, 2), "same", acc=t)
        for pair in ((t, good), (good, t)):
            with pytest.raises(ValueError):
                H.bn_bwd_fin_dual(x, x, 1, [dict(x=x, st=st, acc=a, co=co, dx=x) for a in pair])
    # a valid accumulator passes the check and goes on to the native module
    with pytest.raises(AssertionError, match="native module"):
        H.bn_bwd(x, x, 1, x, st, None, co, x, acc=good)
