"""The launches behind the BatchNorm entry points of ops/hip.py under both statistics protocols
(fp32 partials + finalize launches; int64 accumulators finalized in the consumer): which
bindings are called, in which order, and with which telling arguments.  CPU tensors and a
recording stand-in for the native module: nothing here reaches the device."""
import pytest
import torch

from distributed_amd.ops import hip as H

C, T_BLOCKS = 8, 7
SHAPE = (2, 4, 4, C)
M = 2 * 4 * 4
POOL = ((3, 3), (2, 2), "same")


class Recorder:
    """Every binding records (name, positional, keywords); bn_bwd_blocks answers a constant."""

    def __init__(self):
        self.calls = []

    def bn_bwd_blocks(self, m, c):
        assert (m, c) == (M, C)
        return T_BLOCKS

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append((name, a, k))

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(H, "_C", lambda: r)
    monkeypatch.setattr(H, "stream_handle", lambda: 77)
    return r


def bf():
    return torch.zeros(SHAPE, dtype=torch.bfloat16)


def fin_of(st, reps=3):
    return H.BNFin(H.acc_zeros(reps, 2 * C, "cpu"), torch.ones(C), torch.zeros(C), st, torch.zeros(C), torch.ones(C),
                   M, 1e-3, 0.99)


def bwd_tensors():
    return dict(dy=bf(), y=bf(), x=bf(), st=torch.zeros(4, C), co=torch.zeros(3, C), dx=bf(), dgamma=torch.zeros(C),
                dbeta=torch.zeros(C), part=torch.zeros(T_BLOCKS, 2, C), acc=H.acc_zeros(3, 4 * C, "cpu"))


def p(t):
    return t.data_ptr()


def test_bn_bwd_partials_is_reduce_finalize_apply(rec):
    t = bwd_tensors()
    H.bn_bwd(t["dy"], t["y"], 1, t["x"], t["st"], t["part"], t["co"], t["dx"], dgamma=t["dgamma"], dbeta=t["dbeta"])
    assert rec.names() == ["bn_bwd_reduce", "bn_bwd_finalize", "bn_bwd_apply"]
    (_, red, rk), (_, fz, fk), (_, ap, ak) = rec.calls
    assert red == (p(t["dy"]), p(t["y"]), 1, p(t["x"]), p(t["st"]), 0, p(t["part"]), T_BLOCKS, M, C, 77) and not rk
    assert fz == (p(t["part"]), T_BLOCKS, C, float(M), p(t["st"]), p(t["dgamma"]), p(t["dbeta"]), p(t["co"]), 77)
    assert ap == (p(t["dy"]), p(t["y"]), 1, p(t["x"]), p(t["st"]), p(t["co"]), p(t["dx"]), M, C, 77)
    assert not fk and not ak


def test_bn_bwd_partials_apply_keeps_reading_dy_and_the_mask(rec):
    t, dz = bwd_tensors(), bf()
    H.bn_bwd(t["dy"], t["y"], 1, t["x"], t["st"], t["part"], t["co"], t["dx"], dz_out=dz)
    assert rec.names() == ["bn_bwd_reduce", "bn_bwd_finalize", "bn_bwd_apply"]
    assert rec.calls[0][1][5] == p(dz)
    assert rec.calls[2][1][:3] == (p(t["dy"]), p(t["y"]), 1)


def test_bn_bwd_partials_written_by_a_conv_epilogue(rec):
    """reduce=False: no reduce launch, and T is the row count of the partials offered."""
    t = bwd_tensors()
    part = torch.zeros(5, 2, C)
    H.bn_bwd(t["dy"], None, 2, t["x"], t["st"], part, t["co"], t["dx"], reduce=False)
    assert rec.names() == ["bn_bwd_finalize", "bn_bwd_apply"]
    assert rec.calls[0][1][:3] == (p(part), 5, C)
    assert rec.calls[1][1][:3] == (p(t["dy"]), 0, 2)


def test_bn_bwd_partials_without_dx_has_no_apply(rec):
    t = bwd_tensors()
    H.bn_bwd(t["dy"], None, 0, t["x"], t["st"], t["part"], t["co"], None)
    assert rec.names() == ["bn_bwd_reduce", "bn_bwd_finalize"]


def test_bn_bwd_accumulator_is_reduce_apply(rec):
    t = bwd_tensors()
    H.bn_bwd(t["dy"], t["y"], 1, t["x"], t["st"], None, t["co"], t["dx"], dgamma=t["dgamma"], dbeta=t["dbeta"],
             acc=t["acc"])
    assert rec.names() == ["bn_bwd_reduce", "bn_bwd_apply"]  # no finalize launch
    (_, red, rk), (_, ap, ak) = rec.calls
    assert red == (p(t["dy"]), p(t["y"]), 1, p(t["x"]), p(t["st"]), 0, 0, T_BLOCKS, M, C, 77)  # null partials
    assert rk == dict(acc=p(t["acc"]), reps=3)
    assert ap == (p(t["dy"]), p(t["y"]), 1, p(t["x"]), p(t["st"]), p(t["co"]), p(t["dx"]), M, C, 77)
    assert ak == dict(bfin=[p(t["acc"]), p(t["dgamma"]), p(t["dbeta"]), p(t["co"])], count=float(M), reps=3)


@pytest.mark.parametrize("mask", [1, 2])
def test_bn_bwd_accumulator_apply_reads_the_masked_gradient_just_written(rec, mask):
    t, dz = bwd_tensors(), bf()
    H.bn_bwd(t["dy"], t["y"], mask, t["x"], t["st"], None, t["co"], t["dx"], dz_out=dz, acc=t["acc"])
    assert rec.names() == ["bn_bwd_reduce", "bn_bwd_apply"]
    assert rec.calls[0][1][:6] == (p(t["dy"]), p(t["y"]), mask, p(t["x"]), p(t["st"]), p(dz))
    assert rec.calls[1][1][:3] == (p(dz), 0, 0)  # dz_out as dy, a null mask source, mask 0


def test_bn_bwd_accumulator_other_applies_read_dy(rec):
    t, dz = bwd_tensors(), bf()
    H.bn_bwd(t["dy"], None, 0, t["x"], t["st"], None, t["co"], t["dx"], dz_out=dz, acc=t["acc"])  # no mask
    H.bn_bwd(t["dy"], None, 2, t["x"], t["st"], None, t["co"], t["dx"], acc=t["acc"], reduce=False)  # epilogue sums
    assert rec.names() == ["bn_bwd_reduce", "bn_bwd_apply", "bn_bwd_apply"]
    assert rec.calls[1][1][:3] == (p(t["dy"]), 0, 0)
    assert rec.calls[2][1][:3] == (p(t["dy"]), 0, 2) and rec.calls[2][2]["reps"] == 3


def test_backward_carrier_is_exactly_one_of_part_and_acc(rec):
    t = bwd_tensors()
    for kw in (dict(part=None), dict(part=t["part"], acc=t["acc"])):
        with pytest.raises(ValueError):
            H.bn_bwd(t["dy"], None, 0, t["x"], t["st"], co=t["co"], dx=t["dx"], **kw)
        with pytest.raises(ValueError):
            H.pool_bn_bwd(t["dy"], None, t["x"], t["st"], co=t["co"], dx=t["dx"], pool=POOL[0], strides=POOL[1],
                          padding=POOL[2], **kw)
    assert not rec.calls


def test_pool_bn_bwd_partials(rec):
    t, arg = bwd_tensors(), torch.zeros(2, 2, 2, C, dtype=torch.uint8)
    g = H.pool_geo(SHAPE, *POOL)
    H.pool_bn_bwd(t["dy"], arg, t["x"], t["st"], t["part"], t["co"], t["dx"], *POOL, dgamma=t["dgamma"],
                  dbeta=t["dbeta"])
    assert rec.names() == ["pool_bn_bwd_reduce", "bn_bwd_finalize", "pool_bn_bwd_apply"]
    (_, red, rk), (_, fz, _), (_, ap, ak) = rec.calls
    assert red == (p(t["dy"]), p(arg), g, p(t["x"]), p(t["st"]), p(t["part"]), T_BLOCKS, 77) and not rk
    assert fz == (p(t["part"]), T_BLOCKS, C, float(M), p(t["st"]), p(t["dgamma"]), p(t["dbeta"]), p(t["co"]), 77)
    assert ap == (p(t["dy"]), p(arg), g, p(t["x"]), p(t["st"]), p(t["co"]), p(t["dx"]), 77) and not ak
    rec.calls.clear()
    H.pool_bn_bwd(t["dy"], arg, t["x"], t["st"], t["part"], t["co"], None, *POOL)  # dx None: no apply
    assert rec.names() == ["pool_bn_bwd_reduce", "bn_bwd_finalize"]


def test_pool_bn_bwd_accumulator(rec):
    t, arg = bwd_tensors(), torch.zeros(2, 2, 2, C, dtype=torch.uint8)
    g = H.pool_geo(SHAPE, *POOL)
    H.pool_bn_bwd(t["dy"], arg, t["x"], t["st"], None, t["co"], t["dx"], *POOL, dgamma=t["dgamma"], dbeta=t["dbeta"],
                  acc=t["acc"])
    assert rec.names() == ["pool_bn_bwd_reduce", "pool_bn_bwd_apply"]
    (_, red, rk), (_, ap, ak) = rec.calls
    assert red == (p(t["dy"]), p(arg), g, p(t["x"]), p(t["st"]), 0, T_BLOCKS, 77)
    assert rk == dict(acc=p(t["acc"]), reps=3)
    assert ap == (p(t["dy"]), p(arg), g, p(t["x"]), p(t["st"]), p(t["co"]), p(t["dx"]), 77)
    assert ak == dict(bfin=[p(t["acc"]), p(t["dgamma"]), p(t["dbeta"]), p(t["co"])], count=float(M), reps=3)


@pytest.mark.parametrize("first", ["tensor", "fin"])
@pytest.mark.parametrize("second", [None, "raw", "tensor", "fin"])
def test_bn_apply_takes_a_tensor_or_a_bnfin_in_either_slot(rec, first, second):
    x, y, r = bf(), bf(), bf()
    st, st2 = torch.zeros(4, C), torch.zeros(4, C)
    a = fin_of(st) if first == "fin" else st
    b = {None: None, "raw": None, "tensor": st2, "fin": fin_of(st2, reps=1)}[second]
    H.bn_apply(x, a, y, relu=True, r=None if second is None else r, st2=b)
    (name, pos, kw), = rec.calls
    mode = {None: 0, "raw": 1, "tensor": 2, "fin": 2}[second]
    assert name == "bn_apply"
    assert pos == (p(x), p(st), 0 if second is None else p(r), p(st2) if mode == 2 else 0, mode, 1, p(y), M, C, 77)
    assert set(kw) == {"fin", "fin_v", "fin2", "fin2_v"}
    assert (kw["fin"], kw["fin_v"]) == (a.args() if first == "fin" else ([], []))  # non-empty exactly for a BNFin
    assert (kw["fin2"], kw["fin2_v"]) == (b.args() if second == "fin" else ([], []))
    if first == "fin":
        assert len(kw["fin"]) == 6 and kw["fin"][3] == p(st) and kw["fin_v"] == [float(M), 1e-3, 0.99, 3.0]


@pytest.mark.parametrize("carrier", ["tensor", "fin"])
def test_bn_relu_maxpool_fwd_takes_a_tensor_or_a_bnfin(rec, carrier):
    x, st = bf(), torch.zeros(4, C)
    y, arg = torch.zeros(2, 2, 2, C, dtype=torch.bfloat16), torch.zeros(2, 2, 2, C, dtype=torch.uint8)
    a = fin_of(st) if carrier == "fin" else st
    H.bn_relu_maxpool_fwd(x, a, y, arg, *POOL)
    (name, pos, kw), = rec.calls
    assert name == "bn_relu_maxpool_fwd"
    assert pos == (p(x), p(st), H.pool_geo(SHAPE, *POOL), p(y), p(arg), 77)
    assert (kw["fin"], kw["fin_v"]) == (a.args() if carrier == "fin" else ([], []))
    assert bool(kw["fin"]) == (carrier == "fin")


def test_bn_stats_is_a_partials_reduce_of_x_against_the_identity(rec):
    x, ident, part = bf(), torch.zeros(4, C), torch.zeros(T_BLOCKS, 2, C)
    assert H.bn_stats(x, ident, part) == T_BLOCKS
    assert rec.calls == [("bn_bwd_reduce", (p(x), 0, 0, p(x), p(ident), 0, p(part), T_BLOCKS, M, C, 77), {})]
    with pytest.raises(ValueError):  # no accumulator form: the kernel cannot write the forward layout
        H.bn_stats(x, ident, H.acc_zeros(3, 2 * C, "cpu"))
    assert len(rec.calls) == 1


def test_bn_infer_st_takes_the_channel_count_from_st(rec):
    rm, rv, st = torch.zeros(C), torch.ones(C), torch.zeros(4, C)
    H.bn_infer_st(rm, rv, None, None, 1e-3, st)
    assert rec.calls == [("bn_infer_st", (p(rm), p(rv), 0, 0, 1e-3, C, p(st), 77), {})]
