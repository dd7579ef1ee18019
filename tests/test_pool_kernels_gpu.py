"""Every geometry path of csrc/kernels/pool.hip against the explicit-loop fp64 oracle of
tests/helpers/pool_oracle.py (itself checked against torch in tests/test_pool_oracle.py).

Rectangular images, windows and strides (a swap of ph/pw, sh/sw, pt/pl or Ho/Wo anywhere
between ops/hip.py pool_geo(), the bindings' positional PoolGeo and the kernels shows); all
four <PT, PL> variants of the 2x2-quad stem kernels, through raw geometry lists; the pixel
forward with the quad backward (even H, odd Ho); the in-prologue finalize variants; global
average pooling at its dispatch boundaries; and one case past the launch-grid cap.

The inputs are small integers and the BatchNorm rows / coefficients dyadic, so every fp32
intermediate of the max-pool and stem kernels is exact whatever the summation order or FMA
contraction: those comparisons are bitwise (torch.equal).  Integer activations are full of
tied maxima -- as post-ReLU activations are -- which is where "first in-bounds tap wins" can
go wrong; each test asserts from the oracle that the ties are there.  Average pooling
multiplies by fl(1 / count), so it is held to a derived bound: one bf16 ulp of the result
plus the fp32 accumulation bound, |got - ref| <= 2^-8 |ref| + (taps + 2) 2^-24 mean|x|.
Every output starts as NaN (0xFF for the codes), so an element no thread wrote shows."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from distributed_amd.ops import reference as ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pool_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0") if torch.cuda.is_available() else None
TIE_FLOOR = 0.20


@pytest.fixture(scope="module")
def H():
    from distributed_amd.ops import hip

    return hip


# ---- inputs and oracle results, computed once per geometry ----------------------------------
def ints(shape, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float64)


def cyc(vals, C, shift=0):
    return np.roll(np.resize(np.asarray(vals, dtype=np.float64), C), shift)


def st_rows(C):
    """mean, invstd, scale, shift: dyadic, negative scales included (so "max of x, then
    normalise" picks other taps), cycle lengths 4 / 3 / 5 / 7 so channels differ."""
    return np.stack([cyc([-1, 0, 0.5, 1], C), cyc([0.5, 1, 2], C), cyc([-0.5, 1, -1, 2, 0.5], C),
                     cyc([0, 1, -1, 2, -2, 1, 0], C)])


def co_rows(C):
    return np.stack([cyc([0.5, 1, 2], C), cyc([-1, 0, 0.5], C, 1), cyc([0.25, -0.25, 0.5, -0.25], C)])


@functools.lru_cache(maxsize=None)
def inputs(geo):
    n, h, w, c, ph, pw = geo[:6]
    # (uniform integers: the 2x2 window's maximum over 7 values ties with probability
    # 1 - 4 * 441 / 7^4 = 26.5 %, larger windows more often; the smallest case has 96 (window,
    # channel) pairs, a standard deviation of 4.5 points, so a draw can fall under the floor
    # -- this seed's smallest share is 32 %, and check_ties() asserts it)
    if ph * pw == 255:  # the unique maximum at the last tap: the code must reach 254
        x = ints((n, h, w, c), -3, 2, 104)
        x[:, h - 1, w - 1, :] = 3
    else:
        x = ints((n, h, w, c), -3, 3, 104)
    dp = ints((n, geo[10], geo[11], c), -4, 4, 102)
    return x, dp, st_rows(c), co_rows(c)


@functools.lru_cache(maxsize=None)
def max_ref(geo):
    x, dp, _, _ = inputs(geo)
    y, arg = O.maxpool_fwd(x, geo)
    return y, arg, O.bf16_rne(O.maxpool_bwd(dp, arg, geo)), O.tie_share(x, geo)


@functools.lru_cache(maxsize=None)
def stem_ref(geo):
    x, dp, st, co = inputs(geo)
    y, arg = O.bn_relu_maxpool_fwd(x, st, geo)
    s0, s1, dz = O.pool_bn_bwd(dp, arg, x, st, geo)
    return y, arg, s0, s1, O.pool_bn_bwd_apply(dz, x, st, co), O.tie_share(x, geo, st)


def bf(a):
    """fp64 array of bf16-representable values -> device bf16 (exact)."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    assert torch.equal(t.bfloat16().double(), t)
    return t.bfloat16().to(dev)


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)


def u8(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def nans(shape, dtype=torch.bfloat16):
    return torch.full(tuple(shape), float("nan"), device=dev, dtype=dtype)


def codes(shape):
    return torch.full(tuple(shape), 0xFF, device=dev, dtype=torch.uint8)


def out_shape(geo):
    return (geo[0], geo[10], geo[11], geo[3])


def check_ties(name, geo, share):
    """The tie floor (from the oracle alone) and, where the geometry pads top / left, windows
    whose tap (0, 0) is padding.  Exempt: the 255-tap case (its maximum is unique by
    construction) and a 1x1 window (one tap cannot tie)."""
    outside = O.windows_with_first_tap_outside(geo)
    print(f"\n[pool ties] {name} geo={list(geo)}: tied (window, channel) pairs {100 * share:.1f} %, "
          f"windows with tap (0,0) outside {outside}")
    if geo[4] * geo[5] == 1:
        assert share == 0.0
    elif geo[4] * geo[5] != 255:
        assert share >= TIE_FLOOR, share
    if geo[8] + geo[9] > 0:
        assert outside > 0


TABLE = [pytest.param(*g, id="x".join(map(str, g[0])) + "-p" + "x".join(map(str, g[1])) + "-s"
                      + "x".join(map(str, g[2])) + "-" + g[3]) for g in O.GEOMETRIES]


def run_maxpool(H, geo, hl=None):
    """maxpool_fwd / maxpool_bwd against the oracle, bitwise.  hl: (pool, strides, padding) to
    go through the ops/hip.py wrappers (and pool_geo()); None: the raw geometry list."""
    C_ = H._C()
    x, dp, _, _ = inputs(geo)
    y, arg, dx, share = max_ref(geo)
    check_ties("maxpool", geo, share)
    yo, ao = nans(out_shape(geo)), codes(out_shape(geo))
    dxo = nans(x.shape)
    xb, dpb, argb = bf(x), bf(dp), u8(arg)  # (named: a pointer does not keep its tensor alive)
    if hl is not None:
        H.maxpool_fwd(xb, yo, ao, *hl)
        H.maxpool_bwd(dpb, argb, dxo, *hl)
    else:
        C_.maxpool_fwd(H._ptr(xb), list(geo), H._ptr(yo), H._ptr(ao), H.stream_handle())
        C_.maxpool_bwd(H._ptr(dpb), H._ptr(argb), list(geo), H._ptr(dxo), H.stream_handle())
    assert torch.equal(yo, bf(y))
    assert torch.equal(ao, u8(arg))
    assert torch.equal(dxo, bf(dx))
    if geo[4] * geo[5] == 255:
        assert int(ao.min()) == 254


def run_stem(H, geo, hl=None):
    """bn_relu_maxpool_fwd, pool_bn_bwd_reduce (partials), bn_bwd_finalize's += into dgamma /
    dbeta and pool_bn_bwd_apply (caller-given coefficients) against the oracle, bitwise."""
    C_ = H._C()
    s = H.stream_handle()
    x, dp, st, co = inputs(geo)
    y, arg, s0, s1, dx, share = stem_ref(geo)
    check_ties("stem", geo, share)
    C = geo[3]
    M = geo[0] * geo[1] * geo[2]
    xb, dpb, stf, cof, argb = bf(x), bf(dp), f32(st), f32(co), u8(arg)
    yo, ao = nans(out_shape(geo)), codes(out_shape(geo))
    if hl is not None:
        H.bn_relu_maxpool_fwd(xb, stf, yo, ao, *hl)
    else:
        C_.bn_relu_maxpool_fwd(H._ptr(xb), H._ptr(stf), list(geo), H._ptr(yo), H._ptr(ao), s)
    assert torch.equal(yo, bf(y))
    assert torch.equal(ao, u8(arg))
    T = C_.bn_bwd_blocks(M, C)
    part = nans((T, 2, C), torch.float32)
    C_.pool_bn_bwd_reduce(H._ptr(dpb), H._ptr(argb), list(geo), H._ptr(xb), H._ptr(stf), H._ptr(part), T, s)
    got = part.double().sum(0).cpu()
    assert torch.equal(got[0], torch.from_numpy(s0)), (got[0], s0)
    assert torch.equal(got[1], torch.from_numpy(s1)), (got[1], s1)
    dg, db = torch.ones(C, device=dev), torch.ones(C, device=dev)
    co_fin = nans((3, C), torch.float32)
    C_.bn_bwd_finalize(H._ptr(part), T, C, float(M), H._ptr(stf), H._ptr(dg), H._ptr(db), H._ptr(co_fin), s)
    assert torch.equal(db.double().cpu(), torch.from_numpy(1.0 + s0))
    assert torch.equal(dg.double().cpu(), torch.from_numpy(1.0 + s1))
    assert not torch.isnan(co_fin).any()
    dxo = nans(x.shape)
    C_.pool_bn_bwd_apply(H._ptr(dpb), H._ptr(argb), list(geo), H._ptr(xb), H._ptr(stf), H._ptr(cof), H._ptr(dxo), s)
    assert torch.equal(dxo, bf(dx))


def avg_bound(refv, taps, mabs):
    return 2.0 ** -8 * np.abs(refv) + (taps + 2) * 2.0 ** -24 * mabs


def within(got, refv, bound):
    err = np.abs(got.double().cpu().numpy() - refv)
    assert not np.isnan(err).any()
    assert (err <= bound).all(), f"max excess {(err - bound).max():.3e} at {np.unravel_index((err - bound).argmax(), err.shape)}"


# ---- the geometry table ------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pool,strides,padding", TABLE)
def test_maxpool_geometries(H, shape, pool, strides, padding):
    geo = tuple(O.make_geo(shape, pool, strides, padding))
    assert list(geo) == H.pool_geo(shape, pool, strides, padding)
    run_maxpool(H, geo, (pool, strides, padding))


@pytest.mark.parametrize("shape,pool,strides,padding", TABLE)
def test_avgpool_geometries(H, shape, pool, strides, padding):
    geo = tuple(O.make_geo(shape, pool, strides, padding))
    x, dp, _, _ = inputs(geo)
    y, taps, mabs = O.avgpool_fwd(x, geo, with_bound=True)
    yo = nans(out_shape(geo))
    H.avgpool_fwd(bf(x), yo, pool, strides, padding)
    within(yo, y, avg_bound(y, taps, mabs))
    dx, cover, dabs = O.avgpool_bwd(dp, geo, with_bound=True)
    dxo = nans(shape)
    H.avgpool_bwd(bf(dp), dxo, pool, strides, padding)
    within(dxo, dx, avg_bound(dx, cover, dabs))
    if strides[0] > pool[0]:  # pixels no window covers get exactly 0
        assert (cover == 0).any() and (dxo.double().cpu().numpy()[cover == 0] == 0).all()


@pytest.mark.parametrize("shape,pool,strides,padding", TABLE)
def test_stem_geometries(H, shape, pool, strides, padding):
    run_stem(H, tuple(O.make_geo(shape, pool, strides, padding)), (pool, strides, padding))


# ---- the 3x3 / stride-2 family: all four <PT, PL> kernel variants ---------------------------
@pytest.mark.parametrize("shape", O.QUAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pt,pl", O.QUAD_PADS)
def test_quad_family_stem(H, shape, pt, pl):
    """Ho, Wo both even: quad forward + quad backward; otherwise the pixel forward with the
    quad backward.  TF 'same' only ever gives (pt, pl) = (0, 0) here, so the geometry goes
    to the bindings as a raw list."""
    geo = tuple(O.quad_geo(shape, pt, pl))
    if (pt, pl) == (0, 0):
        assert list(geo) == H.pool_geo(shape, (3, 3), (2, 2), "same")
    run_stem(H, geo)


@pytest.mark.parametrize("shape", O.QUAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pt,pl", O.QUAD_PADS)
def test_quad_family_unfused_maxpool(H, shape, pt, pl):
    run_maxpool(H, tuple(O.quad_geo(shape, pt, pl)))


# ---- windows the uint8 tap code cannot hold --------------------------------------------------
def test_window_of_256_taps_is_refused_before_launch(H):
    C_ = H._C()
    s = H.stream_handle()
    shape, pool = (1, 16, 16, 8), (16, 16)
    geo = O.make_geo(shape, pool, (1, 1), "valid")
    assert geo[4] * geo[5] == 256 and out_shape(geo) == (1, 1, 1, 8)
    x, st, co = bf(ints(shape, -3, 3, 1)), f32(st_rows(8)), f32(co_rows(8))
    dp, arg = bf(ints(out_shape(geo), -4, 4, 2)), torch.zeros(out_shape(geo), device=dev, dtype=torch.uint8)
    y, a, dx = nans(out_shape(geo)), codes(out_shape(geo)), nans(shape)
    part = nans((1, 2, 8), torch.float32)
    with pytest.raises(RuntimeError, match="maxpool_fwd"):
        H.maxpool_fwd(x, y, a, pool, (1, 1), "valid")
    with pytest.raises(RuntimeError, match="bn_relu_maxpool_fwd"):
        H.bn_relu_maxpool_fwd(x, st, y, a, pool, (1, 1), "valid")
    with pytest.raises(RuntimeError, match="maxpool_bwd"):
        H.maxpool_bwd(dp, arg, dx, pool, (1, 1), "valid")
    with pytest.raises(RuntimeError, match="pool_bn_bwd_reduce"):
        C_.pool_bn_bwd_reduce(H._ptr(dp), H._ptr(arg), geo, H._ptr(x), H._ptr(st), H._ptr(part), 1, s)
    with pytest.raises(RuntimeError, match="pool_bn_bwd_apply"):
        C_.pool_bn_bwd_apply(H._ptr(dp), H._ptr(arg), geo, H._ptr(x), H._ptr(st), H._ptr(co), H._ptr(dx), s)
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(dx).all() and torch.isnan(part).all() and bool((a == 0xFF).all())


# ---- finalize in the prologue -------------------------------------------------------------------
FIN_CASES = [pytest.param((4, 16, 24, 64), id="quad"), pytest.param((3, 13, 15, 64), id="pixel")]
FIN_POOL = ((3, 3), (2, 2), "same")


def split_words(words, reps):
    """The accumulator words spread unevenly over the replicas (their integer sum is `words`),
    plus the clear flag row."""
    rows = [torch.full_like(words, 1000 * (r + 1) + 7) * (-1) ** r for r in range(reps - 1)]
    rows.append(words - sum(rows) if rows else words.clone())
    return torch.stack(rows + [torch.zeros_like(words)]).contiguous()


def close64(got, want, rtol, atol):
    got, want = got.double().cpu(), torch.as_tensor(want, dtype=torch.float64)
    err = (got - want).abs()
    assert bool((err <= atol + rtol * want.abs()).all()), f"max abs err {err.max():.3e}"


@pytest.mark.parametrize("reps", [1, 3])
@pytest.mark.parametrize("shape", FIN_CASES)
def test_stem_forward_finalizes_in_its_prologue(H, shape, reps):
    C_ = H._C()
    n, h, w, C = shape
    geo = H.pool_geo(shape, *FIN_POOL)
    M = n * h * w
    x = ints(shape, -3, 3, 201)
    xf = x.reshape(M, C)
    sums = np.concatenate([xf.sum(0), (xf * xf).sum(0)])  # integers: exact at the unit 2^-24
    acc = split_words(H.bn_acc_encode(torch.from_numpy(sums)), reps).to(dev)
    assert acc.shape == (reps + 1, 2 * C) and torch.equal(H.bn_acc_decode(acc), torch.from_numpy(sums))
    gamma, beta = cyc([0.5, -1.5, 1.25, 2, -0.75], C), cyc([0.25, -1, 0, 1.5], C)
    rm0, rv0 = cyc([0.5, -0.25, 1], C), cyc([2, 0.5, 1, 4], C)
    eps, mom = 1e-3, 0.99
    st = nans((4, C), torch.float32)
    rmean, rvar, gd, bd = f32(rm0), f32(rv0), f32(gamma), f32(beta)  # (BNFin keeps pointers, not tensors)
    fin = H.BNFin(acc, gd, bd, st, rmean, rvar, M, eps, mom)
    xb = bf(x)
    y, a = nans(out_shape(geo)), codes(out_shape(geo))
    H.bn_relu_maxpool_fwd(xb, fin, y, a, *FIN_POOL)
    # several blocks: only block 0 publishes st, the others normalise from their own LDS copy
    items = n * geo[10] * geo[11] * C // (32 if geo[10] % 2 == 0 and geo[11] % 2 == 0 else 8)
    assert items > 2 * 256
    mean = sums[:C] / M
    var = sums[C:] / M - mean * mean
    inv = 1.0 / np.sqrt(var + eps)
    want = np.stack([mean, inv, gamma * inv, beta - mean * gamma * inv])
    # bn_finalize's tolerance (test_hip_ops_gpu.py: rtol 1e-5, atol 1e-6 of the largest value)
    for got, w_ in ((st, want), (rmean, rm0 * mom + mean * (1 - mom)), (rvar, rv0 * mom + var * (1 - mom))):
        close64(got, w_, 1e-5, 1e-6 * min(1.0, float(np.abs(w_).max())))
    y2, a2 = nans(out_shape(geo)), codes(out_shape(geo))
    C_.bn_relu_maxpool_fwd(H._ptr(xb), H._ptr(st), geo, H._ptr(y2), H._ptr(a2), H.stream_handle())
    assert torch.equal(y, y2) and torch.equal(a, a2)
    assert not torch.isnan(y).any() and int(a.max()) <= 8


@functools.lru_cache(maxsize=None)
def fin_bwd_ref(geo):
    x, dp, st, _ = inputs(geo)
    _, arg = O.bn_relu_maxpool_fwd(x, st, geo)
    s0, s1, _ = O.pool_bn_bwd(dp, arg, x, st, geo)
    return arg, s0, s1


@pytest.mark.parametrize("reps", [1, 3])
@pytest.mark.parametrize("shape", FIN_CASES)
def test_stem_backward_finalizes_in_its_prologue(H, shape, reps):
    C_ = H._C()
    s = H.stream_handle()
    n, h, w, C = shape
    geo = tuple(H.pool_geo(shape, *FIN_POOL))
    M = n * h * w
    x, dp, st, _ = inputs(geo)
    arg, s0, s1 = fin_bwd_ref(geo)
    xb, dpb, stf, argb = bf(x), bf(dp), f32(st), u8(arg)
    acc = H.acc_zeros(reps, 4 * C, dev)
    T = C_.bn_bwd_blocks(M, C)
    assert T > reps
    C_.pool_bn_bwd_reduce(H._ptr(dpb), H._ptr(argb), list(geo), H._ptr(xb), H._ptr(stf), 0, T, s, acc=H._ptr(acc),
                          reps=reps)
    assert torch.equal(H.bn_acc_decode(acc, 2), torch.from_numpy(np.concatenate([s0, s1])))
    if reps > 1:
        assert bool((acc[:-1] != 0).any(1).all())  # every replica took its blocks' share
    co, dx = nans((3, C), torch.float32), nans(shape)
    dg, db = torch.ones(C, device=dev), torch.ones(C, device=dev)
    C_.pool_bn_bwd_apply(H._ptr(dpb), H._ptr(argb), list(geo), H._ptr(xb), H._ptr(stf), H._ptr(co), H._ptr(dx), s,
                         bfin=[H._ptr(acc), H._ptr(dg), H._ptr(db), H._ptr(co)], count=float(M), reps=reps)
    assert M * C // 8 // 4 > 2 * 256  # several blocks even at one thread per 2x2 quad: LDS copies beyond block 0's
    # three fp32 roundings (the sum, the product, the quotient), 4x margin
    want = np.stack([st[2], -st[2] * s0 / M, -st[2] * s1 / M])
    close64(co, want, 2.0 ** -20, 0.0)
    assert torch.equal(db.double().cpu(), torch.from_numpy(1.0 + s0))
    assert torch.equal(dg.double().cpu(), torch.from_numpy(1.0 + s1))
    dx2 = nans(shape)
    C_.pool_bn_bwd_apply(H._ptr(dpb), H._ptr(argb), list(geo), H._ptr(xb), H._ptr(stf), H._ptr(co), H._ptr(dx2), s)
    assert torch.equal(dx, dx2) and not torch.isnan(dx).any()
    # the wrapper the engine calls: the same two launches
    acc2, co2, dx3 = H.acc_zeros(reps, 4 * C, dev), nans((3, C), torch.float32), nans(shape)
    H.pool_bn_bwd(dpb, argb, xb, stf, None, co2, dx3, *FIN_POOL, acc=acc2)
    assert torch.equal(acc2, acc) and torch.equal(co2, co) and torch.equal(dx3, dx)


# ---- global average pooling ----------------------------------------------------------------------
@pytest.mark.parametrize("n,hw,c", [(3, 63, 24),    # one image per block; 85 pixel groups of 3 threads, thread 255 sits out
                                    (2, 4, 16),     # HW < 8: the generic kernel
                                    (2, 9, 1032),   # 129 channel groups: the generic kernel
                                    (2, 9, 1024)])  # 128 channel groups: the last width of the per-image kernel
def test_gap_dispatch_boundaries(H, n, hw, c):
    x = ints((n, hw, c), -3, 3, 301)
    xb = bf(x).reshape(n, hw, 1, c)
    y = O.gap_fwd(x)
    mabs = np.abs(x).mean(1)
    y32 = nans((n, c), torch.float32)
    H.gap_fwd(xb, y32)
    # integer sums are exact in fp32: fl(1 / HW) and the product round, 2x margin
    within(y32, y, 2.0 ** -22 * np.abs(y))
    y16 = nans((n, c))
    H.gap_fwd(xb, y16)
    within(y16, y, avg_bound(y, hw, mabs))
    dy = ints((n, c), -4, 4, 302)
    want = O.gap_bwd(dy, hw).reshape(n, hw, 1, c)
    for d in (f32(dy), bf(dy)):
        dx = nans((n, hw, 1, c))
        H.gap_bwd(d, dx)
        within(dx, want, avg_bound(want, 1, np.abs(want)))


# ---- beyond the launch-grid cap: the second trip of the grid-stride loops ----------------------
def test_pool_kernels_beyond_the_grid_cap(H):
    """More 8-channel work items than grid_for()'s cap of 8192 blocks x 256 threads, so the
    last items are reached in each thread's second loop trip.  The oracle's loops are too slow
    here: the reference is ops/reference.py on the device (fp32, autograd), and the input is
    tie-free by construction so that torch's gradient routing is unambiguous."""
    shape, pool, strides, padding = (4, 256, 260, 64), (2, 3), (1, 1), "same"
    n, h, w, c = shape
    geo = O.make_geo(shape, pool, strides, padding)
    assert geo[8:] == [0, 1, h, w]
    cap_items = 8192 * 256
    items = n * h * w * c // 8
    assert cap_items < items == 2129920
    ih, iw = torch.arange(h, device=dev) % 2, torch.arange(w, device=dev) % 3
    sc = torch.tensor([1.0, -1.0, 2.0, -2.0], device=dev).repeat(c // 4)
    x = ((3 * ih)[:, None, None] + iw[None, :, None]).float() * sc  # six distinct values in every 2x3 window
    x = x.expand(n, h, w, c).contiguous()
    xs = x[0, :5, :8].cpu()
    for a in range(4):
        for b in range(6):
            win = xs[a:a + 2, b:b + 3].reshape(6, c)
            assert all(len(set(win[:, ch].tolist())) == 6 for ch in range(c))
    g = torch.Generator().manual_seed(401)
    dy = torch.randint(-4, 5, shape, generator=g).float().to(dev)
    xb, dyb = x.bfloat16(), dy.bfloat16()
    assert torch.equal(xb.float(), x)
    # max
    xr = x.clone().requires_grad_(True)
    yr = ref.maxpool2d(xr, pool, strides, padding)
    (gx,) = torch.autograd.grad(yr, (xr,), dy)
    y, a, dx = nans(shape), codes(shape), nans(shape)
    H.maxpool_fwd(xb, y, a, pool, strides, padding)
    H.maxpool_bwd(dyb, a, dx, pool, strides, padding)
    assert torch.equal(y, yr.detach().bfloat16()) and torch.equal(y.float(), yr.detach())
    assert torch.equal(dx.float(), gx)
    assert int(a.max()) <= 5
    del yr, gx, y, a, dx

    # average: the bound's terms from the same reference ops
    def sumpool(t):
        tc = F.pad(t.permute(0, 3, 1, 2), (1, 1, 0, 1))
        return F.avg_pool2d(tc, pool, strides, divisor_override=1).permute(0, 2, 3, 1)

    u = 2.0 ** -24
    xr = x.clone().requires_grad_(True)
    yr = ref.avgpool2d(xr, pool, strides, padding)
    (gx,) = torch.autograd.grad(yr, (xr,), dy)
    taps = sumpool(torch.ones(1, h, w, 1, device=dev))
    assert taps.min() == 2 and taps.max() == 6
    bound = 2.0 ** -8 * yr.detach().abs() + (taps + 2) * u * (sumpool(x.abs()) / taps)
    y = nans(shape)
    H.avgpool_fwd(xb, y, pool, strides, padding)
    assert bool(((y.float() - yr.detach()).abs() <= bound).all())
    one = torch.ones_like(x).requires_grad_(True)
    (cover,) = torch.autograd.grad(sumpool(one), (one,), torch.ones_like(x))
    (sabs,) = torch.autograd.grad(ref.avgpool2d(one, pool, strides, padding), (one,), dy.abs())
    assert cover.min() == 2 and cover.max() == 6
    bound = 2.0 ** -8 * gx.abs() + (cover + 2) * u * (sabs / cover)
    dx = nans(shape)
    H.avgpool_bwd(dyb, dx, pool, strides, padding)
    assert bool(((dx.float() - gx).abs() <= bound).all())
