"""The batch gather, layout and inference glue kernels of csrc/kernels/ (glue.hip,
loss_head.hip, optimizer.hip, bn.hip), called directly: gather_batch (its three code paths, zero ranges, folded PadCastJob, Ctrl::cur3),
pad_cast / unpad_add, logits_store / step_fold / bn_infer_st, add_bf16 / relu_bwd, the
casts and sgd_step.

Almost everything here moves or rounds values without accumulating, so the comparisons are
bitwise against plain torch / numpy on the CPU (bf16 through torch's .bfloat16(), round to
nearest even like f2bf).  Every output buffer is prefilled with a sentinel (0x7fc0 words
for bf16, a large finite constant for fp32 / int32) and carries a guard band of GUARD spare
elements behind the part the kernel may write: a skipped element or a write out of range
fails an assertion.  The two toleranced checks take their bounds from existing tests:
bn_infer_st's fp32 rows as bn_finalize's in test_hip_ops_gpu.py (1e-5, 1e-6; bf16 outputs
1e-2, 5e-3), sgd_step as opt_step in test_native_layers_gpu.py (rtol 1e-5, atol 1e-6 /
1e-7).  The last section runs each grid-stride loop beyond its grid cap (8192 x 256 work
items, 4096 x 256 for sgd_step) with the reference built on the device."""
import struct

import numpy as np
import pytest
import torch

from distributed_amd.engine.ctrl import (C_AC, C_AL, C_AN, C_CUR, C_CUR3, C_GB, C_IT, C_LR, C_MOM, C_NEST, C_NS, C_ROW0,
                                         C_WRAP)
from distributed_amd.ops import reference as ref

dev = torch.device("cuda:0") if torch.cuda.is_available() else None

# words of the device control block (csrc/include/damd_common.h Ctrl)
C_ACC = (C_AL, C_AC, C_AN)  # acc_loss, acc_correct, acc_count

GUARD = 64
BF_SENT = 0x7FC0
F_SENT = 1.0e30
I_SENT = 1_000_000_007
BYTE_SENT = 0xA5
CAP = 8192 * 256  # work items of one trip of the grid-stride loops


@pytest.fixture(scope="module")
def H():
    from distributed_amd.ops import hip

    return hip


@pytest.fixture(scope="module")
def C():
    from distributed_amd.native import require_C

    return require_C()


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def close(a, b, rtol, atol_frac):
    a, b = a.float(), b.float()
    atol = atol_frac * b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"max abs err {err:.3e} (atol {atol:.3e})"


def _ctrl(nsamples, global_batch, row0, cursor, wrap=0, iterations=0, junk=False):
    c = torch.zeros(32, dtype=torch.int32)
    if junk:  # the words no kernel under test may touch are told apart
        c[:] = torch.arange(32, dtype=torch.int32) + 0x1000
    c[C_NS], c[C_GB], c[C_ROW0], c[C_CUR], c[C_WRAP] = nsamples, global_batch, row0, cursor, wrap
    c[C_IT] = iterations
    return c.to(dev)


def _fbits(v):
    return struct.unpack("<i", struct.pack("<f", v))[0]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _sent_bf16(n, device=None):
    return torch.full((n,), BF_SENT, dtype=torch.int16, device=device or dev).view(torch.bfloat16)


def _same_bits(got, want):
    g, w = _bits(got).reshape(-1), _bits(want).reshape(-1).to(got.device)
    assert g.numel() == w.numel()
    bad = (g != w).nonzero()
    assert bad.numel() == 0, f"{bad.numel()} of {g.numel()} words differ, first at {bad[0].item()}"


def _guard_ok(buf, used, sentinel):
    tail = buf.reshape(-1)[used:]
    assert tail.numel() >= GUARD
    if buf.dtype == torch.bfloat16:
        assert torch.all(_bits(tail) == sentinel).item()
    else:
        assert torch.all(tail == sentinel).item()


# ---- references -------------------------------------------------------------------------------
def gather_reference(x, labels, ctrl_words, per, HW, Cin, Cp, scale):
    """The step's rows as gather_batch stores them: (xb bf16 [per][HW][Cp], yb int32 [per]).
    x [n][HW][Cin] fp32 or uint8, labels [n]; ctrl_words the 32 words of Ctrl."""
    w = [int(v) for v in ctrl_words]
    n, gb, row0, cursor, wrap = w[C_NS], w[C_GB], w[C_ROW0], w[C_CUR], w[C_WRAP]
    base = cursor * gb + row0
    r = base + torch.arange(per, device=x.device)
    valid = r < n if wrap <= 0 else torch.ones_like(r, dtype=torch.bool)
    rows = r % n
    x = x.reshape(n, HW, Cin)
    if x.dtype == torch.uint8:  # bf16(float32(k) / float32(scale)), one entry per value of k
        lut = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(scale)).bfloat16().to(x.device)
    out = torch.zeros(per, HW, Cp, dtype=torch.bfloat16, device=x.device)
    for r0 in range(0, per, 16):  # in row chunks: the index tensor of a large case stays small
        src = x[rows[r0:r0 + 16]]
        out[r0:r0 + 16, :, :Cin] = lut[src.long()] if x.dtype == torch.uint8 else src.bfloat16()
    out[~valid] = 0
    yb = torch.where(valid, labels[rows], torch.full_like(labels[rows], -1))
    return out, yb.to(torch.int32)


def pad_cast_reference(src, R, C1, C2, C1p, C2p):
    out = torch.zeros(R, C1p, C2p, dtype=torch.float32, device=src.device)
    out[:, :C1, :C2] = src.reshape(R, C1, C2)
    return out.bfloat16()


# ---- data -------------------------------------------------------------------------------------
def _u8(n, HW, Cin, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, HW, Cin), generator=g, dtype=torch.uint8)
    if x.numel() >= 256:
        x.view(-1)[:256] = torch.randperm(256, generator=g).to(torch.uint8)
    return x


def _f32(n, HW, Cin, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, HW, Cin, generator=g)


def _labels(n):
    return (torch.arange(n, dtype=torch.int32) * 3 + 1) % 1000


def _gather(C, x, labels, ctrl, per, HW, Cin, Cp, scale, **kw):
    """One gather_batch launch into sentinel-filled xb / yb (device tensors in, device out)."""
    xb = _sent_bf16(per * HW * Cp + GUARD)
    yb = torch.full((per + GUARD,), I_SENT, dtype=torch.int32, device=dev)
    C.gather_batch(x.data_ptr(), int(x.dtype == torch.uint8), float(scale), labels.data_ptr(), ctrl.data_ptr(), per,
                   HW, Cin, Cp, xb.data_ptr(), yb.data_ptr(), _stream(), **kw)
    torch.cuda.synchronize()
    return xb, yb


def _check_gather(xb, yb, ctrl, words, x, labels, per, HW, Cin, Cp, scale):
    """xb / yb / ctrl after a launch against gather_reference on the device of x / labels."""
    rx, ry = gather_reference(x, labels, words, per, HW, Cin, Cp, scale)
    nx = per * HW * Cp
    _same_bits(xb[:nx], rx)
    assert torch.equal(yb[:per].to(ry.device), ry)
    _guard_ok(xb, nx, BF_SENT)
    _guard_ok(yb, per, I_SENT)
    want = words.clone()
    want[C_CUR3] = want[C_IT] + 1  # the step's t; the cursor is not advanced
    assert torch.equal(ctrl.cpu(), want.cpu())


# ---- 1. gather_batch --------------------------------------------------------------------------
# (per, HW, Cin, Cp, dtype, scale): the smallest shapes that reach each path's edges
LAYOUTS = []
for _l in [(4, 6, 3, 8), (3, 5, 20, 24), (2, 7, 16, 16)]:  # 8-channel groups
    LAYOUTS += [_l + ("f32", 1.0), _l + ("u8", 255.0), _l + ("u8", 1.0)]
LAYOUTS += [(3, 6, 3, 4, "u8", 255.0), (3, 6, 3, 4, "u8", 1.0),  # two pixels per thread: HW % 4 != 0, no dword path
            (5, 4, 1, 4, "f32", 1.0), (2, 10, 4, 4, "f32", 1.0)]
for _l in [(3, 8, 3, 4), (5, 12, 3, 4)]:  # RGB dword path
    LAYOUTS += [_l + ("u8", 255.0), _l + ("u8", 1.0)]

# (nsamples, global_batch, per or None: the layout's, row0, cursor, wrap)
CURSORS = {
    "layout_per": (40, 8, None, 4, 2, 0),
    "full_rank1": (40, 8, 4, 4, 2, 0),
    "short_final": (22, 8, 4, 4, 2, 0),  # rows 20 and 21 are real
    "past_end": (22, 8, 4, 4, 3, 0),
    "wrap": (10, 8, 8, 0, 1, 5),  # rows 8, 9, 0, 1, ...
}


def _lid(v):
    return "-".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


@pytest.mark.gpu
@pytest.mark.parametrize("cursor", list(CURSORS))
@pytest.mark.parametrize("layout", LAYOUTS, ids=_lid)
def test_gather_batch_rows_padding_labels_and_ctrl(C, layout, cursor):
    per0, HW, Cin, Cp, dt, scale = layout
    n, gb, per, row0, cur, wrap = CURSORS[cursor]
    per = per or per0
    x = (_u8 if dt == "u8" else _f32)(n, HW, Cin, seed=HW * 100 + Cin)
    if dt == "u8" and x.numel() >= 256:
        assert torch.unique(x).numel() == 256
    labels = _labels(n)
    ctrl = _ctrl(n, gb, row0, cur, wrap, iterations=6, junk=True)
    words = ctrl.cpu()
    xb, yb = _gather(C, x.to(dev), labels.to(dev), ctrl, per, HW, Cin, Cp, scale)
    _check_gather(xb, yb, ctrl, words, x, labels, per, HW, Cin, Cp, scale)
    ry = gather_reference(x, labels, words, per, HW, Cin, Cp, scale)[1]
    if cursor == "short_final":
        assert ry.tolist() == [int(labels[20]), int(labels[21]), -1, -1]
    elif cursor == "past_end":
        assert ry.tolist() == [-1] * per
    elif cursor == "wrap":
        assert ry.tolist() == [int(labels[i]) for i in (8, 9, 0, 1, 2, 3, 4, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [255.0, 1.0])
@pytest.mark.parametrize("HW,Cp", [(12, 8), (14, 4), (12, 4)], ids=["groups8", "two_pixel", "rgb_dword"])
def test_gather_batch_uint8_every_value(C, HW, Cp, scale):
    """All 256 byte values inside the gathered rows themselves, on each path."""
    n, per, Cin = 12, 8, 3
    x = _u8(n, HW, Cin, seed=5)
    ctrl = _ctrl(n, per, 2, 0, iterations=1, junk=True)  # rows 2 .. 9
    x[2:10].view(-1)[:256] = torch.randperm(256, generator=torch.Generator().manual_seed(6)).to(torch.uint8)
    assert torch.unique(x[2:10]).numel() == 256
    labels = _labels(n)
    words = ctrl.cpu()
    xb, yb = _gather(C, x.to(dev), labels.to(dev), ctrl, per, HW, Cin, Cp, scale)
    _check_gather(xb, yb, ctrl, words, x, labels, per, HW, Cin, Cp, scale)


def _zero_buf(nbytes, off):
    """A sentinel-filled byte buffer with a range of nbytes at the 16-byte aligned offset off."""
    buf = torch.full((off + nbytes + 4 * GUARD,), BYTE_SENT, dtype=torch.uint8, device=dev)
    assert (buf.data_ptr() + off) % 16 == 0
    return buf


def _zero_ok(buf, nbytes, off):
    b = buf.cpu()
    assert torch.all(b[:off] == BYTE_SENT).item(), "bytes before the range were written"
    assert torch.all(b[off:off + nbytes] == 0).item(), "the range is not all zero"
    assert torch.all(b[off + nbytes:] == BYTE_SENT).item(), "bytes behind the range were written"


@pytest.mark.gpu
@pytest.mark.parametrize("swap", [False, True], ids=["zero_small", "zero_large"])
@pytest.mark.parametrize("shape", [(1, 4, 3, 8), (8, 64, 3, 8), (8, 64, 3, 4)],
                         ids=["tiny_gather", "two_blocks", "rgb_dword"])
def test_gather_batch_zero_ranges(C, shape, swap):
    """The cleared ranges do not depend on the gather's own work size: 1001 16-byte words
    behind a gather of four work items (one block) and of 512."""
    per, HW, Cin, Cp = shape
    n = 16
    x, labels = _u8(n, HW, Cin, seed=7), _labels(n)
    ctrl = _ctrl(n, 8, 0, 1, iterations=3, junk=True)
    words = ctrl.cpu()
    sizes = [16, 16 * 1000 + 16]
    offs = [48, 16]
    if swap:
        sizes.reverse()
    z1, z2 = _zero_buf(sizes[0], offs[0]), _zero_buf(sizes[1], offs[1])
    xb, yb = _gather(C, x.to(dev), labels.to(dev), ctrl, per, HW, Cin, Cp, 255.0, zero=z1.data_ptr() + offs[0],
                     zero_bytes=sizes[0], zero2=z2.data_ptr() + offs[1], zero2_bytes=sizes[1])
    _zero_ok(z1, sizes[0], offs[0])
    _zero_ok(z2, sizes[1], offs[1])
    _check_gather(xb, yb, ctrl, words, x, labels, per, HW, Cin, Cp, 255.0)


PC_JOBS = [(2, 5, 7, 5, 7),  # fewer elements than the smallest gather has threads
           (49, 3, 64, 8, 64),  # more than one block's threads: pc_finish's own stride loop runs
           (7, 7, 3 * 16, 8, 4 * 16)]  # the packed-tap stem form
PC_GATHERS = [(1, 4, 3, 8, "f32"), (3, 6, 3, 4, "u8"), (3, 8, 3, 4, "u8")]  # one launch block each, all three paths


@pytest.mark.gpu
@pytest.mark.parametrize("job", PC_JOBS, ids=_lid)
@pytest.mark.parametrize("gshape", PC_GATHERS, ids=_lid)
def test_gather_batch_folded_pad_cast_job(C, H, gshape, job):
    per, HW, Cin, Cp, dt = gshape
    R, C1, C2, C1p, C2p = job
    n = 8
    x = (_u8 if dt == "u8" else _f32)(n, HW, Cin, seed=9)
    labels = _labels(n)
    ctrl = _ctrl(n, 4, 1, 1, iterations=2, junk=True)
    words = ctrl.cpu()
    src = rnd(R, C1, C2, seed=10)
    total = R * C1p * C2p
    sep = _sent_bf16(total + GUARD)
    H.pad_cast(src, R, C1, C2, C1p, C2p, sep)
    dst = _sent_bf16(total + GUARD)
    xb, yb = _gather(C, x.to(dev), labels.to(dev), ctrl, per, HW, Cin, Cp, 255.0, pc_src=src.data_ptr(),
                     pc_dst=dst.data_ptr(), pc_dims=list(job))
    _same_bits(dst, sep)  # the guard band included
    _same_bits(dst[:total], pad_cast_reference(src.cpu(), *job))
    _guard_ok(dst, total, BF_SENT)
    # the gather's own outputs do not change with the job
    _check_gather(xb, yb, ctrl, words, x, labels, per, HW, Cin, Cp, 255.0)


def _reject_cases():
    # name -> (overrides of the valid call below, layout (per, HW, Cin, Cp))
    return {
        "Cp12": ({}, (2, 4, 3, 12)),
        "Cp4_odd_HW": ({}, (2, 5, 3, 4)),
        "Cp4_Cin5": ({}, (2, 4, 5, 4)),
        "zero_bytes8": ({"zero_off": 0, "zero_bytes": 8}, (2, 4, 3, 8)),
        "zero_ptr_plus8": ({"zero_off": 8, "zero_bytes": 16}, (2, 4, 3, 8)),
        "pc_C1p_below_C1": ({"pc_dims": [2, 5, 7, 4, 7], "pc_dst": True}, (2, 4, 3, 8)),
        "pc_null_dst": ({"pc_dims": [2, 5, 7, 5, 7], "pc_dst": False}, (2, 4, 3, 8)),
        "rgb_x_plus1": ({"x_off": 1}, (3, 8, 3, 4)),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_reject_cases()))
def test_gather_batch_rejects_before_any_launch(C, name):
    over, (per, HW, Cin, Cp) = _reject_cases()[name]
    n = 8
    x = torch.zeros(n * HW * Cin + 16, dtype=torch.uint8, device=dev)  # room for the shifted pointer
    labels = _labels(n).to(dev)
    ctrl = _ctrl(n, 4, 0, 0, iterations=4, junk=True)
    words = ctrl.cpu()
    xb = _sent_bf16(per * HW * 16 + GUARD)
    yb = torch.full((per + GUARD,), I_SENT, dtype=torch.int32, device=dev)
    zbuf = torch.full((256,), BYTE_SENT, dtype=torch.uint8, device=dev)
    src = rnd(2 * 5 * 7, seed=11)
    dst = _sent_bf16(2 * 5 * 7 + GUARD)
    kw = {}
    if "zero_bytes" in over:
        kw.update(zero=zbuf.data_ptr() + over["zero_off"], zero_bytes=over["zero_bytes"])
    if "pc_dims" in over:
        kw.update(pc_src=src.data_ptr(), pc_dst=dst.data_ptr() if over["pc_dst"] else 0, pc_dims=over["pc_dims"])
    with pytest.raises(RuntimeError):
        C.gather_batch(x.data_ptr() + over.get("x_off", 0), 1, 255.0, labels.data_ptr(), ctrl.data_ptr(), per, HW,
                       Cin, Cp, xb.data_ptr(), yb.data_ptr(), _stream(), **kw)
    torch.cuda.synchronize()
    assert torch.all(_bits(xb) == BF_SENT).item() and torch.all(yb == I_SENT).item()
    assert torch.all(zbuf == BYTE_SENT).item() and torch.all(_bits(dst) == BF_SENT).item()
    assert torch.equal(ctrl.cpu(), words)  # cur3 included: nothing ran


# ---- 2. pad_cast / unpad_add ------------------------------------------------------------------
PAD_SHAPES = [(9, 3, 64, 8, 64), (1, 50, 10, 50, 16), (7, 7, 48, 8, 64), (2, 5, 7, 5, 7)]


def _check_pad_cast(H, shape, on_device=False):
    R, C1, C2, C1p, C2p = shape
    src = rnd(R, C1, C2, seed=20)
    total = R * C1p * C2p
    dst = _sent_bf16(total + GUARD)
    H.pad_cast(src, R, C1, C2, C1p, C2p, dst)
    torch.cuda.synchronize()
    want = pad_cast_reference(src if on_device else src.cpu(), *shape)
    _same_bits(dst[:total], want)
    got = dst[:total].reshape(R, C1p, C2p)
    assert torch.all(_bits(got[:, C1:, :]) == 0).item() and torch.all(_bits(got[:, :, C2:]) == 0).item()
    _guard_ok(dst, total, BF_SENT)


def _check_unpad_add(H, shape, on_device=False):
    R, C1, C2, C1p, C2p = shape
    src = torch.full((R, C1p, C2p), float("nan"), device=dev)  # NaN in every padded position: none is read
    inner = rnd(R, C1, C2, seed=21)
    src[:, :C1, :C2] = inner
    total = R * C1 * C2
    dst = torch.full((total + GUARD,), F_SENT, device=dev)
    dst0 = rnd(total, seed=22)
    dst[:total] = dst0
    where = (lambda t: t) if on_device else (lambda t: t.cpu())
    want = where(dst0) + where(inner).reshape(-1)  # one fp32 add per element
    H.unpad_add(src, R, C1, C2, C1p, C2p, dst)
    torch.cuda.synchronize()
    assert torch.equal(where(dst[:total]), want)
    H.unpad_add(src, R, C1, C2, C1p, C2p, dst)  # a second call adds again
    torch.cuda.synchronize()
    assert torch.equal(where(dst[:total]), want + where(inner).reshape(-1))
    _guard_ok(dst, total, F_SENT)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PAD_SHAPES, ids=_lid)
def test_pad_cast_is_bitwise_and_zero_pads(H, shape):
    _check_pad_cast(H, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PAD_SHAPES, ids=_lid)
def test_unpad_add_reads_no_padding_and_adds_once(H, shape):
    _check_unpad_add(H, shape)


# ---- 3. logits_store / step_fold --------------------------------------------------------------
def _check_logits_store(C, B, K, ld, n, gb, row0, cur):
    z = rnd(B, ld, seed=30)
    z[:, K:] = float("nan")  # pad columns must not appear in out
    ctrl = _ctrl(n, gb, row0, cur, iterations=5, junk=True)
    words = ctrl.cpu()
    out = torch.full(((n + B) * K + GUARD,), F_SENT, device=dev)
    C.logits_store(z.data_ptr(), ld, K, B, ctrl.data_ptr(), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    want = torch.full(((n + B) * K + GUARD,), F_SENT)
    base = cur * gb + row0
    real = [r for r in range(B) if base + r < n]
    for r in real:
        want[(base + r) * K:(base + r + 1) * K] = z[r, :K].cpu()
    assert torch.equal(out.cpu(), want)  # nothing else changes, nothing at or past row n
    assert torch.equal(ctrl.cpu(), words)
    return real


@pytest.mark.gpu
@pytest.mark.parametrize("case,n,cur,nreal", [("full", 40, 2, 5), ("short_final", 22, 2, 2), ("past_end", 22, 3, 0)])
def test_logits_store_writes_only_real_rows(C, case, n, cur, nreal):
    assert len(_check_logits_store(C, 5, 10, 16, n, 8, 4, cur)) == nreal


@pytest.mark.gpu
def test_logits_store_imagenet_head(C):
    assert len(_check_logits_store(C, 64, 1000, 1000, 100, 64, 0, 1)) == 36


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["K0", "B0", "null_ctrl", "K_above_ld"])
def test_logits_store_rejects_before_any_launch(C, case):
    B, K, ld = 5, 10, 16
    z = rnd(B, ld, seed=31)
    ctrl = _ctrl(40, 8, 0, 0)
    out = torch.full((45 * 32 + GUARD,), F_SENT, device=dev)
    args = {"K0": (ld, 0, B, ctrl.data_ptr()), "B0": (ld, K, 0, ctrl.data_ptr()), "null_ctrl": (ld, K, B, 0),
            "K_above_ld": (ld, ld + 1, B, ctrl.data_ptr())}[case]
    with pytest.raises(RuntimeError):
        C.logits_store(z.data_ptr(), args[0], args[1], args[2], args[3], out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert torch.all(out == F_SENT).item()


def _ctrl_f(ctrl, i):
    return ctrl.cpu().view(torch.float32)[i].item()


@pytest.mark.gpu
@pytest.mark.parametrize("wrap,cur,nxt", [(0, 4, 5), (5, 3, 4), (5, 4, 0), (0, 0, 1)])
def test_step_fold_accumulates_clears_and_advances(C, wrap, cur, nxt):
    ctrl = _ctrl(100, 8, 0, cur, wrap, iterations=9, junk=True)
    acc0 = [1.5, 2.0, 64.0]
    for i, v in zip(C_ACC, acc0):
        ctrl[i] = _fbits(v)
    words = ctrl.cpu()
    tail = torch.tensor([3.25, 5.0, 8.0, F_SENT], device=dev)
    t0 = tail.cpu()
    C.step_fold(ctrl.data_ptr(), tail.data_ptr(), _stream())
    torch.cuda.synchronize()
    acc1 = [np.float32(a) + np.float32(t) for a, t in zip(acc0, t0[:3].tolist())]
    assert [_ctrl_f(ctrl, i) for i in C_ACC] == acc1
    assert tail.cpu()[:3].tolist() == [0.0, 0.0, 0.0]  # cleared for the next step
    assert tail.cpu()[3].item() == t0[3].item()  # and nothing behind it
    want = words.clone()
    want[C_CUR] = nxt
    for i, v in zip(C_ACC, acc1):
        want[i] = _fbits(float(v))
    assert torch.equal(ctrl.cpu(), want)  # every other word unchanged
    # a second fold accumulates
    tail[:3] = torch.tensor([0.125, 1.0, 8.0], device=dev)
    C.step_fold(ctrl.data_ptr(), tail.data_ptr(), _stream())
    torch.cuda.synchronize()
    acc2 = [a + np.float32(t) for a, t in zip(acc1, [0.125, 1.0, 8.0])]
    assert [_ctrl_f(ctrl, i) for i in C_ACC] == acc2
    assert tail.cpu()[:3].tolist() == [0.0, 0.0, 0.0]
    # a null tail: the accumulators stay, the cursor still moves
    before = ctrl.cpu()
    C.step_fold(ctrl.data_ptr(), 0, _stream())
    torch.cuda.synchronize()
    c = int(before[C_CUR]) + 1
    before[C_CUR] = 0 if wrap > 0 and c >= wrap else c
    assert torch.equal(ctrl.cpu(), before)


# ---- 4. bn_infer_st ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("has_beta", [True, False])
@pytest.mark.parametrize("has_gamma", [True, False])
@pytest.mark.parametrize("Cn", [8, 48, 300, 304])
def test_bn_infer_st_rows_and_bn_apply(C, H, Cn, has_gamma, has_beta):
    """300: more than one block and no multiple of the block size.  bn_apply takes NHWC bf16
    activations whose channel count is a multiple of 8 (layer_ops.h), so the apply half runs
    at 8, 48 and 304 (304 stands in for 300 there)."""
    eps = 1e-3
    rmean = rnd(Cn, seed=40)
    rvar = rnd(Cn, seed=41).abs() + 0.1
    rvar[0], rvar[Cn - 1] = 0.0, 1.0e6
    gamma = rnd(Cn, seed=42).abs() + 0.5 if has_gamma else None
    beta = rnd(Cn, seed=43) if has_beta else None
    st = torch.full((4 * Cn + GUARD,), F_SENT, device=dev)
    C.bn_infer_st(rmean.data_ptr(), rvar.data_ptr(), gamma.data_ptr() if has_gamma else 0,
                  beta.data_ptr() if has_beta else 0, eps, Cn, st.data_ptr(), _stream())
    torch.cuda.synchronize()
    m, v = rmean.cpu().double(), rvar.cpu().double()
    inv = 1.0 / torch.sqrt(v + eps)
    sc = (gamma.cpu().double() if has_gamma else torch.ones(Cn, dtype=torch.float64)) * inv
    sh = (beta.cpu().double() if has_beta else torch.zeros(Cn, dtype=torch.float64)) - m * sc
    got = st[:4 * Cn].cpu().reshape(4, Cn)
    assert torch.equal(got[0], rmean.cpu())  # the mean row is a copy
    close(got[1], inv, 1e-5, 1e-6)
    close(got[2], sc, 1e-5, 1e-6)
    close(got[3], sh, 1e-5, 1e-6)
    _guard_ok(st, 4 * Cn, F_SENT)  # the four floats behind st[4 * C] among them
    if Cn % 8:
        return
    x = (rnd(2, 3, 3, Cn, seed=44) * 2 + 0.5).bfloat16()
    y = torch.empty_like(x)
    H.bn_apply(x, st[:4 * Cn].reshape(4, Cn), y, relu=True)
    g1 = gamma.cpu() if has_gamma else torch.ones(Cn)
    b1 = beta.cpu() if has_beta else torch.zeros(Cn)
    yr = ref.batchnorm(x.float().cpu(), g1, b1, rmean.cpu(), rvar.cpu(), False, 0.99, eps).relu()
    close(y.cpu(), yr, 1e-2, 5e-3)


# ---- 5. elementwise and casts -----------------------------------------------------------------
def _bf_rand(n, seed, scale=1.0):
    return rnd(n, seed=seed, scale=scale).bfloat16()


def _check_add_bf16(H, n, on_device=False):
    where = (lambda t: t) if on_device else (lambda t: t.cpu())
    a, b = _bf_rand(n, 50, 2.0), _bf_rand(n, 51)
    out = _sent_bf16(n + GUARD)
    H.add_bf16(a, b, out[:n])
    torch.cuda.synchronize()
    want = (where(a).float() + where(b).float()).bfloat16()
    _same_bits(where(out[:n]), want)
    _guard_ok(out, n, BF_SENT)
    acc = a.clone()  # in place, as the residual-gradient accumulation calls it
    H.add_bf16(acc, b, acc)
    torch.cuda.synchronize()
    _same_bits(where(acc), want)


def _relu_bwd_case(n, seed):
    """(dy, y) bf16 on the device: y random with the edge patterns spread through it."""
    y = _bits(_bf_rand(n, seed)).clone()
    edge = torch.tensor([0x0000, -0x8000, 0x0001, -0x7FFF, 0x7F80, -0x0080, -0x4080, 0x0080],
                        dtype=torch.int16, device=dev)  # +0 -0 +denorm_min -denorm_min +inf -inf -1.0 +norm_min
    for k in range(0, n, 1009):
        m = min(edge.numel(), n - k)
        y[k:k + m] = edge[:m]
    dy = _bf_rand(n, seed + 1) + 0.25  # finite; zero nowhere the edges sit with overwhelming odds
    dy = torch.where(dy == 0, torch.ones_like(dy), dy)
    return dy.contiguous(), y.view(torch.bfloat16)


def _check_relu_bwd(H, n, on_device=False):
    where = (lambda t: t) if on_device else (lambda t: t.cpu())
    dy, y = _relu_bwd_case(n, 52)
    dz = _sent_bf16(n + GUARD)
    H.relu_bwd(dy, y, dz[:n])
    torch.cuda.synchronize()
    want = torch.where(where(y).float() > 0, where(dy), torch.zeros_like(where(dy)))  # +0.0 where masked
    _same_bits(where(dz[:n]), want)
    _guard_ok(dz, n, BF_SENT)
    return want


@pytest.mark.gpu
def test_add_bf16_bitwise_in_place_and_rejects(H):
    _check_add_bf16(H, 8 * 1000)
    n = 8 * 1000 + 4
    a, b = _bf_rand(n, 53), _bf_rand(n, 54)
    out = _sent_bf16(n + GUARD)
    with pytest.raises(RuntimeError):
        H.add_bf16(a, b, out[:n])
    torch.cuda.synchronize()
    assert torch.all(_bits(out) == BF_SENT).item()


@pytest.mark.gpu
def test_relu_bwd_mask_edges_bitwise_and_rejects(H):
    want = _check_relu_bwd(H, 8 * 1000)
    # the mask at the edge values: +0, -0 -> 0; the smallest subnormal and +inf pass dy
    dy, y = _relu_bwd_case(8 * 1000, 52)
    w = _bits(want)[:8].tolist()
    d = _bits(dy.cpu())[:8].tolist()
    assert w == [0, 0, d[2], 0, d[4], 0, 0, d[7]]
    assert all(v != 0 for v in d)
    n = 8 * 1000 + 3
    dz = _sent_bf16(n + GUARD)
    with pytest.raises(RuntimeError):
        H.relu_bwd(_bf_rand(n, 55), _bf_rand(n, 56), dz[:n])
    torch.cuda.synchronize()
    assert torch.all(_bits(dz) == BF_SENT).item()


@pytest.mark.gpu
def test_cast_bf16_f32_every_bit_pattern(C):
    b = np.arange(65536, dtype=np.uint32)
    x = torch.from_numpy(b.astype(np.uint16).view(np.int16)).to(dev)
    y = torch.full((65536 + GUARD,), F_SENT, device=dev)
    C.cast_bf16_f32(x.data_ptr(), y.data_ptr(), 65536, _stream())
    torch.cuda.synchronize()
    got = y[:65536].cpu().numpy().view(np.uint32)
    nan = ((b & 0x7F80) == 0x7F80) & ((b & 0x7F) != 0)
    assert np.array_equal(got[~nan], (b << 16)[~nan])
    assert np.isnan(got[nan].view(np.float32)).all() and nan.sum() == 254
    _guard_ok(y, 65536, F_SENT)


def _cast_f32_inputs():
    """Every finite bf16 value b, just below / at / just above the midpoint to the next bf16
    value of larger magnitude, and the special values (fp32 bit patterns)."""
    b = np.arange(65536, dtype=np.uint32)
    b = b[(b & 0x7F80) != 0x7F80] << 16
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x00400000,
                        0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00008001, 0x00007FFF], dtype=np.uint32)
    big = np.array([3.4e38, -3.4e38], dtype=np.float32).view(np.uint32)  # beyond the largest bf16: inf
    return np.concatenate([b, b | 0x7FFF, b | 0x8000, b | 0x8001, special, big])


def _check_cast_f32_bf16(H, x, n, on_device=False):
    y = _sent_bf16(n + GUARD)
    H.cast_bf16(x[:n], y[:n])
    torch.cuda.synchronize()
    if on_device:
        _same_bits(y[:n], x[:n].bfloat16())
    else:
        _same_bits(y[:n].cpu(), x[:n].cpu().bfloat16())
    _guard_ok(y, n, BF_SENT)


@pytest.mark.gpu
def test_cast_f32_bf16_round_to_nearest_even(H):
    bits = _cast_f32_inputs()
    assert bits.size == 4 * (65536 - 256) + 14
    xf = torch.from_numpy(bits.view(np.float32).copy())
    assert not torch.isnan(xf).any()
    want = xf.bfloat16()
    # the oracle itself: ties go to the even bf16 value, 3.4e38 rounds to inf
    nb = 65536 - 256
    tie = _bits(want)[2 * nb:3 * nb].numpy().view(np.uint16).astype(np.uint32)
    src = bits[:nb] >> 16
    assert np.array_equal(tie, src + (src & 1))
    assert torch.isinf(want[-2:]).all()
    _check_cast_f32_bf16(H, xf.to(dev), xf.numel())


@pytest.mark.gpu
def test_cast_f32_bf16_odd_length(H):
    _check_cast_f32_bf16(H, rnd(1003, seed=57, scale=3.0), 1003)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 1.0 / 255.0])
def test_cast_u8_bf16_multiplies(C, scale):
    # cast_u8_bf16 MULTIPLIES by scale (bf16(float32(k) * float32(scale))); gather_batch DIVIDES
    # by its scale (bf16(float32(k) / float32(scale))).  k * (1/255) and k / 255 differ in the
    # last fp32 bit for some k, so the two are not interchangeable.
    x = torch.arange(256, dtype=torch.int32).to(torch.uint8).to(dev)
    y = _sent_bf16(256 + GUARD)
    C.cast_u8_bf16(x.data_ptr(), float(scale), y.data_ptr(), 256, _stream())
    torch.cuda.synchronize()
    want = torch.from_numpy(np.arange(256, dtype=np.float32) * np.float32(scale)).bfloat16()
    _same_bits(y[:256].cpu(), want)
    _guard_ok(y, 256, BF_SENT)


# ---- 6. sgd_step ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,momentum,nesterov", [("plain", 0.0, False), ("momentum", 0.9, False),
                                                    ("nesterov", 0.9, True)])
def test_sgd_step_matches_apply_flat(C, name, momentum, nesterov):
    """Three consecutive steps against the Keras SGD's own fp32 apply_flat on the CPU; lr and
    momentum come from ctrl, and block 0 keeps the step's books."""
    import distributed_amd as tf

    n = 10007
    torch.manual_seed(3)
    opt = tf.keras.optimizers.SGD(learning_rate=0.05, momentum=momentum, nesterov=nesterov)
    opt.ensure_slots(n, torch.device("cpu"))
    p0 = torch.randn(n)
    ph = p0.clone()
    P = torch.full((n + GUARD,), F_SENT, device=dev)
    P[:n] = p0.to(dev)
    V = torch.full((n + GUARD,), F_SENT, device=dev)
    V[:n] = 0
    Pb = _sent_bf16(n + GUARD)
    ctrl = _ctrl(1000, 8, 0, 1, wrap=3, iterations=5, junk=True)
    ctrl[C_LR], ctrl[C_MOM], ctrl[C_NEST] = _fbits(0.05), _fbits(momentum), int(nesterov)
    for i in C_ACC:
        ctrl[i] = 0
    acc = [np.float32(0)] * 3
    cursors = [2, 0, 1]  # from 1, modulo wrap = 3
    for step, lr in enumerate([0.05, 0.02, 0.02]):
        g = torch.randn(n) * (0.1 if step % 2 else 1.0) + 0.05
        gd = g.to(dev)
        ctrl[C_LR] = _fbits(lr)  # a new rate is a new word of ctrl and nothing else
        opt.learning_rate = lr
        tail = torch.tensor([1.25 + step, 3.0 * step, 8.0], device=dev)
        words = ctrl.cpu()
        C.sgd_step(P.data_ptr(), gd.data_ptr(), V.data_ptr() if momentum else 0, Pb.data_ptr(), n, ctrl.data_ptr(),
                   tail.data_ptr(), _stream())
        torch.cuda.synchronize()
        opt.apply_flat(ph, g)
        torch.testing.assert_close(P[:n].cpu(), ph, rtol=1e-5, atol=1e-6)
        if momentum:
            torch.testing.assert_close(V[:n].cpu(), opt.slots["momentum"], rtol=1e-5, atol=1e-7)
        else:
            assert torch.all(V[:n] == 0).item()
        _same_bits(Pb[:n], P[:n].bfloat16())
        for buf, s in ((P, F_SENT), (V, F_SENT), (Pb, BF_SENT)):
            _guard_ok(buf, n, s)
        # the books: accumulators gain the tail (which stays), cursor and iterations advance
        assert tail.cpu().tolist() == [1.25 + step, 3.0 * step, 8.0]
        acc = [a + np.float32(t) for a, t in zip(acc, [1.25 + step, 3.0 * step, 8.0])]
        want = words.clone()
        want[C_CUR], want[C_IT] = cursors[step], 5 + step + 1
        for i, v in zip(C_ACC, acc):
            want[i] = _fbits(float(v))
        assert torch.equal(ctrl.cpu(), want)
    assert opt.iterations == 3


# ---- 7. beyond the grid cap -------------------------------------------------------------------
# One case per grid-stride loop whose second trip nothing else reaches; references on the device.
@pytest.mark.gpu
@pytest.mark.parametrize("per,HW,Cin,Cp,items", [(33, 4096, 3, 128, 33 * 4096 * 16), (65, 65538, 3, 4, 65 * 65538 // 2),
                                                 (129, 65536, 3, 4, 129 * 65536 // 4)],
                         ids=["groups8", "two_pixel", "rgb_dword"])
def test_gather_batch_beyond_grid_cap(C, per, HW, Cin, Cp, items):
    assert items > CAP
    n = 7  # wrap mode: every row is real, the rows of the second trip hold data
    x = _u8(n, HW, Cin, seed=60).to(dev)
    labels = _labels(n).to(dev)
    ctrl = _ctrl(n, per, 2, 1, wrap=5, iterations=11, junk=True)
    words = ctrl.cpu()
    xb, yb = _gather(C, x, labels, ctrl, per, HW, Cin, Cp, 255.0)
    _check_gather(xb, yb, ctrl, words, x, labels, per, HW, Cin, Cp, 255.0)


@pytest.mark.gpu
def test_sgd_step_beyond_grid_cap(C):
    n = 4096 * 256 + 1003
    lr, mom = 0.05, 0.9
    p0, g, v0 = rnd(n, seed=61), rnd(n, seed=62), rnd(n, seed=63, scale=0.1)
    P = torch.full((n + GUARD,), F_SENT, device=dev)
    V = torch.full((n + GUARD,), F_SENT, device=dev)
    P[:n], V[:n] = p0, v0
    Pb = _sent_bf16(n + GUARD)
    ctrl = _ctrl(1000, 8, 0, 0, iterations=0)
    ctrl[C_LR], ctrl[C_MOM] = _fbits(lr), _fbits(mom)
    tail = torch.zeros(3, device=dev)
    C.sgd_step(P.data_ptr(), g.data_ptr(), V.data_ptr(), Pb.data_ptr(), n, ctrl.data_ptr(), tail.data_ptr(), _stream())
    torch.cuda.synchronize()
    vr = v0.clone().mul_(mom).add_(g, alpha=-lr)  # SGD.apply_flat's expression
    pr = p0.clone().add_(vr)
    torch.testing.assert_close(P[:n], pr, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(V[:n], vr, rtol=1e-5, atol=1e-7)
    _same_bits(Pb[:n], P[:n].bfloat16())
    for buf, s in ((P, F_SENT), (V, F_SENT), (Pb, BF_SENT)):
        _guard_ok(buf, n, s)
    assert int(ctrl[C_IT]) == 1 and int(ctrl[C_CUR]) == 1


# padded total = 8192 * 256 + 8 * 64 (pad_cast's loop); unpadded total the same (unpad_add's)
CAP_PAD_SHAPES = [(4097, 3, 50, 8, 64), (4097, 8, 64, 8, 72)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CAP_PAD_SHAPES, ids=_lid)
def test_pad_cast_unpad_add_beyond_grid_cap(H, shape):
    R, C1, C2, C1p, C2p = shape
    assert R * C1p * C2p >= CAP + 8 * 64 and (R * C1p * C2p == CAP + 8 * 64 or R * C1 * C2 == CAP + 8 * 64)
    _check_pad_cast(H, shape, on_device=True)
    _check_unpad_add(H, shape, on_device=True)


@pytest.mark.gpu
def test_add_bf16_relu_bwd_beyond_grid_cap(H):
    n = 8 * (CAP + 77)
    _check_add_bf16(H, n, on_device=True)
    _check_relu_bwd(H, n, on_device=True)


@pytest.mark.gpu
def test_casts_beyond_grid_cap(C, H):
    n = CAP + 1003
    x = rnd(n, seed=64, scale=3.0)
    _check_cast_f32_bf16(H, x, n, on_device=True)
    xb = x.bfloat16()
    y = torch.full((n + GUARD,), F_SENT, device=dev)
    C.cast_bf16_f32(xb.data_ptr(), y.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    assert torch.equal(y[:n].view(torch.int32), _bits(xb).to(torch.int32) << 16)
    _guard_ok(y, n, F_SENT)


# ---- 8. the oracles, on the CPU ---------------------------------------------------------------
def _ctrl_words(nsamples, global_batch, row0, cursor, wrap=0):
    c = torch.zeros(32, dtype=torch.int32)
    c[C_NS], c[C_GB], c[C_ROW0], c[C_CUR], c[C_WRAP] = nsamples, global_batch, row0, cursor, wrap
    return c


def _gather_loops(cursor, dt, scale):
    per, HW, Cin, Cp = 3, 4, 3, 8
    n, gb, _, row0, cur, wrap = CURSORS[cursor]
    x = (_u8 if dt == "u8" else _f32)(n, HW, Cin, seed=70)
    labels = _labels(n)
    gx, gy = gather_reference(x, labels, _ctrl_words(n, gb, row0, cur, wrap), per, HW, Cin, Cp, scale)
    assert gx.shape == (per, HW, Cp) and gx.dtype == torch.bfloat16 and gy.dtype == torch.int32
    for i in range(per):
        g = cur * gb + row0 + i
        real = wrap > 0 or g < n
        assert int(gy[i]) == (int(labels[g % n]) if real else -1)
        for p in range(HW):
            for c in range(Cp):
                if real and c < Cin:
                    k = x[g % n, p, c]
                    v = np.float32(int(k)) / np.float32(scale) if dt == "u8" else np.float32(float(k))
                    want = torch.tensor(float(v), dtype=torch.float32).bfloat16()
                else:
                    want = torch.zeros((), dtype=torch.bfloat16)
                assert _bits(gx[i, p, c].reshape(1)).item() == _bits(want.reshape(1)).item(), (i, p, c)
    if cursor == "short_final":  # rows 20, 21 and one past the end
        assert gy.tolist() == [int(labels[20]), int(labels[21]), -1] and torch.all(_bits(gx[2]) == 0).item()
    if cursor == "wrap":
        assert gy.tolist() == [int(labels[i]) for i in (8, 9, 0)]


def test_references_against_explicit_loops():
    """gather_reference against a triple loop written from gather_batch's header comment
    (csrc/include/layer_ops.h): row = (cursor * global_batch + row0 + i) mod nsamples; past
    the end of the data (no wrap) the image is zero and the label -1; channels >= Cin zero.
    pad_cast_reference against its loop.  Runs without a GPU."""
    for cursor in ("short_final", "wrap", "full_rank1", "past_end"):
        for dt, scale in (("f32", 1.0), ("u8", 255.0), ("u8", 1.0)):
            _gather_loops(cursor, dt, scale)
    # pad_cast: dst[r][c1][c2] = bf16(src[r][c1][c2]) inside, zero in the padding
    R, C1, C2, C1p, C2p = 2, 3, 5, 4, 8
    src = torch.randn(R, C1, C2, generator=torch.Generator().manual_seed(71))
    got = pad_cast_reference(src, R, C1, C2, C1p, C2p)
    assert got.shape == (R, C1p, C2p) and got.dtype == torch.bfloat16
    for r in range(R):
        for c1 in range(C1p):
            for c2 in range(C2p):
                want = src[r, c1, c2].bfloat16() if c1 < C1 and c2 < C2 else torch.zeros((), dtype=torch.bfloat16)
                assert _bits(got[r, c1, c2].reshape(1)).item() == _bits(want.reshape(1)).item()
