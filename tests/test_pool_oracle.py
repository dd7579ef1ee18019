"""The pooling oracle of tests/helpers/pool_oracle.py against plain PyTorch (ops/reference.py,
fp64 autograd on the CPU) -- what tests/test_pool_kernels_gpu.py compares the HIP kernels
with must itself be right.  Integer inputs: full of tied maxima, and every sum is exact, so
the comparisons are equalities."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_amd.ops import hip as H
from distributed_amd.ops import reference as ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pool_oracle as O  # noqa: E402


def ints(shape, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float64)


@pytest.mark.parametrize("shape,pool,strides,padding", O.GEOMETRIES)
def test_geometry_matches_pool_geo(shape, pool, strides, padding):
    assert O.make_geo(shape, pool, strides, padding) == H.pool_geo(shape, pool, strides, padding)


@pytest.mark.parametrize("shape,pool,strides,padding", O.GEOMETRIES)
def test_maxpool_oracle_matches_torch(shape, pool, strides, padding):
    geo = O.make_geo(shape, pool, strides, padding)
    x = ints(shape, -3, 3, 1)
    assert O.tie_share(x, geo) > 0.2 or pool == (1, 1)  # ties are what the routing is about
    y, arg = O.maxpool_fwd(x, geo)
    xt = torch.from_numpy(x).requires_grad_(True)
    yt = ref.maxpool2d(xt, pool, strides, padding)
    assert torch.equal(torch.from_numpy(y), yt.detach())
    dy = ints(y.shape, -4, 4, 2)
    (gx,) = torch.autograd.grad(yt, (xt,), torch.from_numpy(dy))
    assert torch.equal(torch.from_numpy(O.maxpool_bwd(dy, arg, geo)), gx)
    # the code is the tap of the first maximum: x at that tap is y, and no earlier tap equals it
    ph, pw, sh, sw, pt, pl = geo[4:10]
    for n in range(shape[0]):
        for oh in range(geo[10]):
            for ow in range(geo[11]):
                for c in range(0, shape[3], 5):
                    k = int(arg[n, oh, ow, c])
                    ih, iw = oh * sh - pt + k // pw, ow * sw - pl + k % pw
                    assert x[n, ih, iw, c] == y[n, oh, ow, c]
                    for j in range(k):
                        jh, jw = oh * sh - pt + j // pw, ow * sw - pl + j % pw
                        if 0 <= jh < shape[1] and 0 <= jw < shape[2]:
                            assert x[n, jh, jw, c] < y[n, oh, ow, c]


@pytest.mark.parametrize("shape", O.QUAD_SHAPES)
@pytest.mark.parametrize("pt,pl", O.QUAD_PADS)
def test_maxpool_oracle_explicit_padding_matches_torch(shape, pt, pl):
    geo = O.quad_geo(shape, pt, pl)
    x = ints(shape, -3, 3, 3)
    y, arg = O.maxpool_fwd(x, geo)
    xt = torch.from_numpy(x).requires_grad_(True)
    xc = xt.permute(0, 3, 1, 2)
    if (pt, pl) == (1, 1):
        yt = F.max_pool2d(xc, 3, 2, padding=1)
    else:  # 3x3 / stride 2 over 2 Ho rows from row -pt: 1 - pt rows past the end
        yt = F.max_pool2d(F.pad(xc, (pl, 1 - pl, pt, 1 - pt), value=float("-inf")), 3, 2)
    yt = yt.permute(0, 2, 3, 1)
    assert tuple(yt.shape) == y.shape and torch.equal(torch.from_numpy(y), yt.detach())
    dy = ints(y.shape, -4, 4, 4)
    (gx,) = torch.autograd.grad(yt, (xt,), torch.from_numpy(dy))
    assert torch.equal(torch.from_numpy(O.maxpool_bwd(dy, arg, geo)), gx)
    # windows whose first tap is padding: the code still counts taps from the window's corner
    assert (O.windows_with_first_tap_outside(geo) > 0) == (pt + pl > 0)


@pytest.mark.parametrize("shape,pool,strides,padding", O.GEOMETRIES)
def test_avgpool_oracle_matches_torch(shape, pool, strides, padding):
    geo = O.make_geo(shape, pool, strides, padding)
    x = ints(shape, -3, 3, 5)
    y, taps, mabs = O.avgpool_fwd(x, geo, with_bound=True)
    xt = torch.from_numpy(x).requires_grad_(True)
    yt = ref.avgpool2d(xt, pool, strides, padding)
    assert torch.allclose(torch.from_numpy(y), yt.detach(), rtol=1e-14, atol=1e-14)
    dy = ints(y.shape, -4, 4, 6)
    (gx,) = torch.autograd.grad(yt, (xt,), torch.from_numpy(dy))
    dx, cover, dabs = O.avgpool_bwd(dy, geo, with_bound=True)
    assert torch.allclose(torch.from_numpy(dx), gx, rtol=1e-14, atol=1e-14)
    # the bound's terms: taps / mean |x| of the forward, covering windows of the backward
    assert taps.min() >= 1 and taps.max() <= pool[0] * pool[1]
    assert torch.allclose(torch.from_numpy(mabs), ref.avgpool2d(xt.detach().abs(), pool, strides, padding), atol=1e-14)
    # (every window hands each of its pixels 1 / taps: taps times that, summed, counts the windows)
    one = torch.ones(shape, dtype=torch.float64, requires_grad=True)
    means = ref.avgpool2d(one, pool, strides, padding)
    (cv,) = torch.autograd.grad(means, (one,), torch.from_numpy(taps))
    assert torch.equal(torch.from_numpy(cover), cv.round()) and (cv - cv.round()).abs().max() < 1e-12
    (da,) = torch.autograd.grad(ref.avgpool2d(one, pool, strides, padding), (one,), torch.from_numpy(np.abs(dy)))
    assert torch.allclose(torch.from_numpy(dabs * cover), da, atol=1e-14)
    if strides[0] > pool[0]:
        assert (cover == 0).any() and (dx[cover == 0] == 0).all()


def test_stem_oracle_is_bn_relu_then_pool():
    """bn_relu_maxpool_fwd / pool_bn_bwd of the oracle == its own unfused steps with torch's
    BN arithmetic in between, on a geometry with negative scales (max(x) then normalise
    would pick other taps)."""
    shape, pool, strides, padding = O.GEOMETRIES[4]
    geo = O.make_geo(shape, pool, strides, padding)
    C = shape[-1]
    x = ints(shape, -3, 3, 7)
    st = np.stack([np.resize([-1, 0, 0.5, 1], C), np.resize([0.5, 1, 2], C), np.resize([-0.5, 1, -1, 2, 0.5], C),
                   np.resize([1, -2, 0, 2, -1], C)]).astype(np.float64)
    z = torch.from_numpy(x) * torch.from_numpy(st[2]) + torch.from_numpy(st[3])
    z = z.relu().bfloat16().double().numpy()
    y, arg = O.bn_relu_maxpool_fwd(x, st, geo)
    y0, arg0 = O.maxpool_fwd(z, geo)
    assert np.array_equal(y, y0) and np.array_equal(arg, arg0)
    y1, arg1 = O.maxpool_fwd(x, geo)
    assert not np.array_equal(arg, arg1)
    dp = ints(y.shape, -4, 4, 8)
    s0, s1, dz = O.pool_bn_bwd(dp, arg, x, st, geo)
    dz0 = np.where(z > 0, O.maxpool_bwd(dp, arg, geo), 0.0)
    assert np.array_equal(dz, dz0)
    xhat = (x - st[0]) * st[1]
    assert np.array_equal(s0, dz0.reshape(-1, C).sum(0)) and np.array_equal(s1, (dz0 * xhat).reshape(-1, C).sum(0))
    co = np.stack([np.resize([0.5, 1, 2], C), np.resize([-1, 0, 0.5], C), np.resize([0.25, -0.25, 0.5], C)])
    assert np.array_equal(O.pool_bn_bwd_apply(dz, x, st, co), co[0] * dz + co[1] + co[2] * xhat)  # exact in bf16


def test_gap_oracle():
    x = ints((3, 63, 24), -3, 3, 9)
    assert np.allclose(O.gap_fwd(x), x.mean(1), rtol=1e-15, atol=1e-15)
    dy = ints((3, 24), -4, 4, 10)
    dx = O.gap_bwd(dy, 63)
    assert dx.shape == (3, 63, 24) and np.array_equal(dx, np.broadcast_to((dy / 63)[:, None], dx.shape))


def test_bf16_rne_matches_torch():
    g = torch.Generator().manual_seed(11)
    v = torch.randn(20000, generator=g) * torch.tensor(2.0) ** torch.randint(-30, 30, (20000,), generator=g)
    # exact ties (the 9th significant bit set, nothing below), both parities of the kept bits
    m = torch.arange(128, 256, dtype=torch.float32)
    ties = torch.cat([(m + 0.5) * s for s in (1.0, -1.0, 2.0 ** -20, 2.0 ** 40)])
    # the edges: subnormals, the largest finite value and the overflow tie, signed zeros
    edge = torch.tensor([0.0, -0.0, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -126, 3.3895314e38,
                         float.fromhex("0x1.ffp127"), float.fromhex("0x1.fefffep127"), float("inf"), -float("inf")])
    for t in (v, ties, edge):
        got = torch.from_numpy(O.bf16_rne(t.double().numpy()))
        want = t.bfloat16().double()
        assert torch.equal(got, want)
        assert torch.equal(torch.signbit(got), torch.signbit(want))
    assert np.isnan(O.bf16_rne(np.array([np.nan]))[0])
    # one rounding straight from fp64: just above a tie rounds up although fp32 would see the tie
    assert O.bf16_rne(np.array([1.0 + 2.0 ** -8 + 2.0 ** -40]))[0] == 1.0 + 2.0 ** -7
    assert O.bf16_rne(np.array([1.0 + 2.0 ** -8]))[0] == 1.0


def test_bn_acc_encode_decode_round_trips_integer_sums():
    g = torch.Generator().manual_seed(12)
    C = 24
    sums = torch.randint(-(2 ** 30), 2 ** 30, (2 * C,), generator=g).double()
    for words in (1, 2):
        enc = H.bn_acc_encode(sums, words)
        assert enc.dtype == torch.int64 and enc.shape == (2 * C * words,)
        acc = torch.zeros(4, enc.numel(), dtype=torch.int64)  # 3 replicas + the flag row
        acc[0], acc[1], acc[2] = enc - 12345, torch.full_like(enc, 345), torch.full_like(enc, 12000)
        assert torch.equal(H.bn_acc_decode(acc, words), sums)
        assert torch.equal(H.bn_acc_decode(torch.cat([enc, torch.zeros_like(enc)]), words), sums)
    # quarter-integer sums (the stem backward's sum dz*xhat) need the two-word form's low plane
    q = (sums % 1024) / 4 + 2.0 ** -30
    assert torch.equal(H.bn_acc_decode(torch.stack([H.bn_acc_encode(q, 2), torch.zeros(4 * C, dtype=torch.int64)]), 2), q)
    # a set flag poisons its channel, in both statistics
    acc = torch.stack([H.bn_acc_encode(sums, 1), torch.zeros(2 * C, dtype=torch.int64)])
    acc[1, 3] = 1
    out = H.bn_acc_decode(acc, 1)
    assert torch.isnan(out[3]) and torch.isnan(out[C + 3]) and torch.isnan(out).sum() == 2
