"""engine/ctrl.py against ``struct Ctrl`` of csrc/include/damd_common.h: the word indices the
host writes and reads are the members' positions in the header, so a member inserted there
fails here instead of corrupting training silently."""
import math
import os
import re

from distributed_amd.engine import ctrl

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "include", "damd_common.h")


def _members():
    """[(type, name, array length or None, leading number of the comment or None)]"""
    src = open(HEADER).read()
    body = re.search(r"struct\s+Ctrl\s*\{(.*?)\n\};", src, re.S).group(1)
    out = []
    for line in body.splitlines():
        m = re.match(r"\s*(\w+)\s+(\w+)(?:\[(\d+)\])?\s*;\s*(?://\s*(\d+)\b)?", line)
        if m:
            out.append((m.group(1), m.group(2), int(m.group(3)) if m.group(3) else None,
                        int(m.group(4)) if m.group(4) else None))
        else:
            assert not line.strip() or line.strip().startswith("//"), line  # a comment's continuation
    return out


def test_fields_are_the_header_members_in_order():
    mem = _members()
    assert all(t in ("float", "int") for t, _, _, _ in mem), mem
    assert mem[-1][1:3] == ("pad", 6)
    named = mem[:-1]
    assert all(n is None for _, _, n, _ in named)  # one word each
    assert tuple(nm for _, nm, _, _ in named) == ctrl.FIELDS
    assert len(ctrl.FIELDS) + 6 == ctrl.WORDS == 32
    for i, (_, nm, _, num) in enumerate(named):
        assert num == i, (nm, num, i)  # the index in the member's comment


def test_word_indices():
    assert ctrl.C_LR == 0
    assert ctrl.C_IT == 7
    assert (ctrl.C_AL, ctrl.C_AC, ctrl.C_AN) == (10, 11, 12)
    assert ctrl.C_WRAP == 13
    assert ctrl.C_CUR3 == 15
    assert ctrl.C_BAD == 20
    assert ctrl.C_XGEN == 25
    # every C_* constant is a distinct word of a named field
    idx = sorted(v for k, v in vars(ctrl).items() if k.startswith("C_"))
    assert idx == list(range(len(ctrl.FIELDS)))


def test_float_bits_round_trip():
    import numpy as np

    assert ctrl.i2f(ctrl.f2i(0.1)) == float(np.float32(0.1))
    assert ctrl.f2i(0.1) == 0x3DCCCCCD
    z = ctrl.i2f(ctrl.f2i(-0.0))
    assert z == 0.0 and math.copysign(1.0, z) == -1.0
    assert ctrl.f2i(-0.0) == -2 ** 31
    assert ctrl.i2f(ctrl.f2i(float("inf"))) == float("inf") and ctrl.f2i(float("inf")) == 0x7F800000
    nan_bits = 0x7FC00123  # a quiet NaN with a payload
    assert math.isnan(ctrl.i2f(nan_bits)) and ctrl.f2i(ctrl.i2f(nan_bits)) == nan_bits


def test_helpers_name_the_words_the_engines_write():
    assert ctrl.hparam_words(0.5, 0.9, True) == {0: ctrl.f2i(0.5), 1: ctrl.f2i(0.9), 2: 1}
    assert ctrl.epoch_start_words(7) == {6: 0, 10: 0, 11: 0, 12: 0, 13: 7}
    w = [0] * 32
    w[10], w[11], w[12] = ctrl.f2i(6.0), ctrl.f2i(3.0), ctrl.f2i(4.0)
    assert ctrl.epoch_metrics(w, ["accuracy"]) == {"loss": 1.5, "_count": 4.0, "accuracy": 0.75}
    assert ctrl.epoch_metrics(w, ["acc"], tail=[2.0, 1.0, 4.0]) == {"loss": 1.0, "_count": 8.0, "acc": 0.5}
    w[20] = 1
    assert ctrl.epoch_metrics(w, [])["loss"] == 1.5  # the graph engine does not read `bad`
    assert math.isnan(ctrl.epoch_metrics(w, [], check_bad=True)["loss"])
    assert ctrl.epoch_metrics([0] * 32, ["accuracy"]) == {"loss": 0.0, "_count": 0.0, "accuracy": 0.0}
