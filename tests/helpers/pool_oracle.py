"""Explicit-loop fp64 host oracle of csrc/kernels/pool.hip (numpy only).

Every function takes the 12-int geometry list of ops/hip.py pool_geo()
``[N, H, W, C, ph, pw, sh, sw, pt, pl, Ho, Wo]`` -- so paddings pool_geo() never produces
(pt = pl = 1 on an even image) are covered too -- and NHWC fp64 arrays.  The loops walk every
(image, window, tap) one at a time; only the channel axis, over which every operation is
elementwise, is a numpy vector.  Window (oh, ow) starts at input pixel (oh*sh - pt,
ow*sw - pl); taps outside the image do not exist (they neither win a max nor count in an
average).

Conventions of the kernels reproduced here: the max is the FIRST in-bounds tap, in row-major
(kh, kw) order, that is strictly greater than every earlier one, stored as the code
``kh*pw + kw`` (uint8); bf16 outputs are rounded to nearest even; the fused stem rounds every
candidate relu(x*scale + shift) to bf16 before comparing, and its backward rounds the routed
pool gradient to bf16 before the ReLU mask."""
import numpy as np


# The geometries of tests/test_pool_oracle.py (oracle against torch on the CPU) and
# tests/test_pool_kernels_gpu.py (kernels against the oracle): input shape, pool, strides,
# padding -- everything Keras can express ...
GEOMETRIES = [
    ((2, 7, 10, 24), (2, 3), (1, 2), "same"),   # everything rectangular; 3 channel groups in a 256-thread block
    ((2, 9, 6, 8), (3, 2), (2, 1), "valid"),
    ((1, 8, 11, 8), (2, 2), (3, 3), "valid"),   # stride > window: pixels no window covers
    ((2, 5, 5, 8), (5, 5), (1, 1), "same"),     # pt = pl = 2, every window overhangs
    ((2, 7, 9, 8), (3, 3), (2, 2), "same"),     # pt = pl = 1 on the pixel-centric kernels
    ((2, 4, 6, 40), (1, 1), (2, 2), "valid"),
    ((1, 15, 17, 8), (15, 17), (1, 1), "valid"),  # 255 taps: the largest window the uint8 code holds
]
# ... and the 3x3 / stride-2 pool with H = 2 Ho, W = 2 Wo under all four (pt, pl), of which
# TF 'same' only gives (0, 0): raw geometry lists
QUAD_SHAPES = [(2, 8, 12, 16), (2, 6, 10, 24), (1, 8, 6, 8)]
QUAD_PADS = [(0, 0), (1, 1), (1, 0), (0, 1)]


def same_pad(size, k, s):
    """(out, pad before) of TF 'same' padding: the odd pixel goes after."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return out, total // 2


def make_geo(shape, pool, strides, padding):
    """The 12-int geometry list, worked out here and not by the code under test."""
    n, h, w, c = shape
    if padding == "same":
        ho, pt = same_pad(h, pool[0], strides[0])
        wo, pl = same_pad(w, pool[1], strides[1])
    elif padding == "valid":
        ho, pt = (h - pool[0]) // strides[0] + 1, 0
        wo, pl = (w - pool[1]) // strides[1] + 1, 0
    else:
        raise ValueError(padding)
    return [n, h, w, c, pool[0], pool[1], strides[0], strides[1], pt, pl, ho, wo]


def quad_geo(shape, pt, pl):
    n, h, w, c = shape
    assert h % 2 == 0 and w % 2 == 0
    return [n, h, w, c, 3, 3, 2, 2, pt, pl, h // 2, w // 2]


def bf16_rne(a):
    """fp64 -> the nearest bfloat16 value (8 significant bits, ties to even, subnormals of
    unit 2^-133, overflow to inf), returned as fp64; one rounding straight from fp64."""
    a = np.asarray(a, dtype=np.float64)
    out = a.copy()
    fin = np.isfinite(a)
    _, e = np.frexp(np.where(fin, a, 0.0))  # |a| in [2^(e-1), 2^e)
    q = np.ldexp(1.0, np.maximum(e, -125) - 8)
    r = np.rint(np.where(fin, a, 0.0) / q) * q  # power-of-two scaling is exact; rint ties to even
    big = np.abs(r) > (2.0 - 2.0 ** -7) * 2.0 ** 127
    r = np.where(big, np.copysign(np.inf, r), r)
    out[fin] = r[fin]
    return out


def _geo(geo):
    if len(geo) != 12:
        raise ValueError("geo: [N, H, W, C, ph, pw, sh, sw, pt, pl, Ho, Wo]")
    return [int(v) for v in geo]


def _windows(geo):
    N, H, W, C, ph, pw, sh, sw, pt, pl, Ho, Wo = _geo(geo)
    for n in range(N):
        for oh in range(Ho):
            for ow in range(Wo):
                yield n, oh, ow


def _taps(geo, oh, ow):
    """In-bounds taps of window (oh, ow): (kh, kw, ih, iw) in row-major order."""
    N, H, W, C, ph, pw, sh, sw, pt, pl, Ho, Wo = _geo(geo)
    out = []
    for kh in range(ph):
        ih = oh * sh - pt + kh
        if ih < 0 or ih >= H:
            continue
        for kw in range(pw):
            iw = ow * sw - pl + kw
            if iw < 0 or iw >= W:
                continue
            out.append((kh, kw, ih, iw))
    return out


def _check_x(x, geo):
    N, H, W, C = _geo(geo)[:4]
    x = np.asarray(x, dtype=np.float64)
    if x.shape != (N, H, W, C):
        raise ValueError(f"input {x.shape} against geo {(N, H, W, C)}")
    return x


def _check_y(y, geo):
    g = _geo(geo)
    y = np.asarray(y)
    if y.shape != (g[0], g[10], g[11], g[3]):
        raise ValueError(f"pooled tensor {y.shape} against geo {(g[0], g[10], g[11], g[3])}")
    return y


def _max_scan(cand, geo):
    """(y, arg, tied) of the candidates [N, H, W, C]; tied: the maximum occurs at >= 2 taps."""
    g = _geo(geo)
    C, pw, Ho, Wo = g[3], g[5], g[10], g[11]
    y = np.full((g[0], Ho, Wo, C), -np.inf)
    arg = np.zeros((g[0], Ho, Wo, C), dtype=np.uint8)
    tied = np.zeros((g[0], Ho, Wo, C), dtype=bool)
    for n, oh, ow in _windows(geo):
        best = np.full(C, -np.inf)
        code = np.zeros(C, dtype=np.int64)
        hits = np.zeros(C, dtype=np.int64)
        for kh, kw, ih, iw in _taps(geo, oh, ow):
            v = cand[n, ih, iw]
            for c in range(C):
                if v[c] > best[c]:
                    best[c], code[c], hits[c] = v[c], kh * pw + kw, 1
                elif v[c] == best[c]:
                    hits[c] += 1
        y[n, oh, ow], arg[n, oh, ow], tied[n, oh, ow] = best, code.astype(np.uint8), hits > 1
    return y, arg, tied


def maxpool_fwd(x, geo):
    y, arg, _ = _max_scan(_check_x(x, geo), geo)
    return y, arg


def _route(dy, arg, geo):
    """Sum over the windows covering each input pixel whose stored code is that pixel's tap."""
    g = _geo(geo)
    pw = g[5]
    dy = _check_y(dy, geo).astype(np.float64)
    arg = _check_y(arg, geo)
    dx = np.zeros((g[0], g[1], g[2], g[3]))
    for n, oh, ow in _windows(geo):
        for kh, kw, ih, iw in _taps(geo, oh, ow):
            for c in range(g[3]):
                if int(arg[n, oh, ow, c]) == kh * pw + kw:
                    dx[n, ih, iw, c] += dy[n, oh, ow, c]
    return dx


def maxpool_bwd(dy, arg, geo):
    return _route(dy, arg, geo)


def avgpool_fwd(x, geo, with_bound=False):
    """Mean over the in-bounds taps.  with_bound: also (taps, mean |x| over the taps) per
    element, the terms of the fp32 accumulation bound."""
    x = _check_x(x, geo)
    g = _geo(geo)
    y = np.zeros((g[0], g[10], g[11], g[3]))
    taps = np.zeros(y.shape)
    mabs = np.zeros(y.shape)
    for n, oh, ow in _windows(geo):
        t = _taps(geo, oh, ow)
        s = np.zeros(g[3])
        sa = np.zeros(g[3])
        for kh, kw, ih, iw in t:
            s = s + x[n, ih, iw]
            sa = sa + np.abs(x[n, ih, iw])
        y[n, oh, ow] = s / len(t)
        taps[n, oh, ow] = len(t)
        mabs[n, oh, ow] = sa / len(t)
    return (y, taps, mabs) if with_bound else y


def avgpool_bwd(dy, geo, with_bound=False):
    """dx = sum over the covering windows of dy / (that window's in-bounds taps).
    with_bound: also (covering windows, mean |dy / taps| over them) per element."""
    g = _geo(geo)
    dy = _check_y(dy, geo).astype(np.float64)
    dx = np.zeros((g[0], g[1], g[2], g[3]))
    cover = np.zeros(dx.shape)
    sabs = np.zeros(dx.shape)
    for n, oh, ow in _windows(geo):
        t = _taps(geo, oh, ow)
        for kh, kw, ih, iw in t:
            dx[n, ih, iw] += dy[n, oh, ow] / len(t)
            cover[n, ih, iw] += 1
            sabs[n, ih, iw] += np.abs(dy[n, oh, ow]) / len(t)
    return (dx, cover, sabs / np.maximum(cover, 1)) if with_bound else dx


def _st(st, C):
    st = np.asarray(st, dtype=np.float64)
    if st.shape != (4, C):
        raise ValueError("st: [4, C] rows mean, invstd, scale, shift")
    return st


def _bn_relu(x, st):
    return bf16_rne(np.maximum(x * st[2] + st[3], 0.0))


def bn_relu_maxpool_fwd(x, st, geo):
    x = _check_x(x, geo)
    y, arg, _ = _max_scan(_bn_relu(x, _st(st, x.shape[-1])), geo)
    return y, arg


def tie_share(x, geo, st=None):
    """Share of the (window, channel) pairs whose maximum is attained by two or more
    in-bounds taps (of x, or of the stem's candidates when st is given)."""
    x = _check_x(x, geo)
    cand = x if st is None else _bn_relu(x, _st(st, x.shape[-1]))
    return float(_max_scan(cand, geo)[2].mean())


def windows_with_first_tap_outside(geo):
    """Number of windows (n, oh, ow) whose tap (0, 0) lies in the padding."""
    g = _geo(geo)
    k = 0
    for n, oh, ow in _windows(geo):
        ih, iw = oh * g[6] - g[8], ow * g[7] - g[9]
        k += not (0 <= ih < g[1] and 0 <= iw < g[2])
    return k


def pool_bn_bwd(dpool, arg, x, st, geo):
    """(sum dz, sum dz*xhat) per channel and dz [N, H, W, C]: the pool gradient routed by arg,
    rounded to bf16, masked by relu(bn(x)) > 0; xhat = (x - mean) * invstd."""
    x = _check_x(x, geo)
    st = _st(st, x.shape[-1])
    d = bf16_rne(_route(dpool, arg, geo))
    dz = np.where(_bn_relu(x, st) > 0.0, d, 0.0)
    xhat = (x - st[0]) * st[1]
    return dz.sum(axis=(0, 1, 2)), (dz * xhat).sum(axis=(0, 1, 2)), dz


def pool_bn_bwd_apply(dz, x, st, co):
    """dx = a*dz + b + c*xhat rounded to bf16; co: [3, C] rows a, b, c."""
    x = np.asarray(x, dtype=np.float64)
    st = _st(st, x.shape[-1])
    co = np.asarray(co, dtype=np.float64)
    return bf16_rne(co[0] * dz + co[1] + co[2] * ((x - st[0]) * st[1]))


def gap_fwd(x):
    """x [N, HW, C] -> the mean over HW, [N, C]."""
    x = np.asarray(x, dtype=np.float64)
    s = np.zeros((x.shape[0], x.shape[2]))
    for p in range(x.shape[1]):
        s = s + x[:, p]
    return s / x.shape[1]


def gap_bwd(dy, HW):
    """dy [N, C] -> dx [N, HW, C] = dy / HW at every pixel."""
    dy = np.asarray(dy, dtype=np.float64)
    dx = np.zeros((dy.shape[0], HW, dy.shape[1]))
    for p in range(HW):
        dx[:, p] = dy / HW
    return dx
