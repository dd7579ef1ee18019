"""The Ctrl block on the host (csrc/include/damd_common.h ``struct Ctrl``): 32 int32 words,
the host/device contract of every step kernel, of gather_batch, opt_step and the loss heads.

The one place the word layout is written down in Python; tests/test_ctrl_layout.py checks
it against the header.  Floats travel as their bit patterns (``f2i`` / ``i2f``).  The
helpers are pure, but for ``rmw``, around which each engine keeps its own synchronisation.
"""
import struct

# the members of struct Ctrl before `pad`, in header order
FIELDS = ("lr", "momentum", "nesterov", "nsamples", "row0", "global_batch", "cursor", "iterations", "cnt_a", "cnt_b",
          "acc_loss", "acc_correct", "acc_count", "wrap", "cur2", "cur3", "wpar", "flush_ticket", "pending", "par2",
          "bad", "xcnt", "xcnt2", "ticket", "pend2", "xgen")
WORDS = 32
# word indices, one per field (C_CUR3: the step's `t` for the graph engine's kernels)
(C_LR, C_MOM, C_NEST, C_NS, C_ROW0, C_GB, C_CUR, C_IT, C_CA, C_CB, C_AL, C_AC, C_AN, C_WRAP, C_CUR2, C_CUR3, C_WPAR,
 C_FLUSHT, C_PEND, C_PAR2, C_BAD, C_XCNT, C_XCNT2, C_TICKET, C_PEND2, C_XGEN) = range(len(FIELDS))


def f2i(f: float) -> int:
    return struct.unpack("<i", struct.pack("<f", float(f)))[0]


def i2f(i: int) -> float:
    return struct.unpack("<f", struct.pack("<i", int(i)))[0]


def hparam_words(lr, momentum=0.0, nesterov=False) -> dict:
    return {C_LR: f2i(lr), C_MOM: f2i(momentum), C_NEST: int(nesterov)}


def epoch_start_words(wrap_steps: int = 0) -> dict:
    """Cursor and the epoch accumulators to zero; ``wrap_steps > 0``: the cursor wraps."""
    return {C_CUR: 0, C_AL: 0, C_AC: 0, C_AN: 0, C_WRAP: int(wrap_steps)}


def epoch_metrics(words, names, tail=None, check_bad=False) -> dict:
    """An engine's metrics(): mean loss, count, the accuracy under each of ``names``.  ``tail``: a pending
    step's sums (fused engine).  ``check_bad``: a non-finite / out-of-range value met a fixed-point sum
    (ctrl.bad): the loss is NaN, like the fp32 engines would show it (TerminateOnNaN must fire)."""
    loss, corr, cnt = (i2f(words[k]) for k in (C_AL, C_AC, C_AN))
    if tail is not None:
        loss, corr, cnt = loss + tail[0], corr + tail[1], cnt + tail[2]
    d = max(cnt, 1.0)
    out = {"loss": float("nan") if check_bad and words[C_BAD] else loss / d, "_count": cnt}
    for nm in names:
        out[nm] = corr / d
    return out


def rmw(ctrl, updates: dict, bump_xgen: bool = False) -> None:
    """Read-modify-write of the device block ``ctrl`` through the host (the caller syncs).
    ``bump_xgen``: a batch the last bwd prefetched must not match its tag any more."""
    c = ctrl.cpu()
    for k, v in updates.items():
        c[k] = v
    if bump_xgen:
        c[C_XGEN] = (int(c[C_XGEN]) + 1) & 0x7fffffff
    ctrl.copy_(c.to(ctrl.device))
