"""Explicit-loop fp64 host oracle of csrc/kernels/dwconv.hip (numpy only): depthwise
convolution with depth_multiplier 1, its backprop-input, weight gradient and bias gradient.

Every function takes the 12-int geometry list of ops/hip.py pool_geo()
``[N, H, W, C, kh, kw, sh, sw, pt, pl, Ho, Wo]`` and NHWC fp64 arrays; the taps are
``w[kh, kw, C]``.  The loops walk every (output row, tap) one at a time and list the output
columns whose tap lands inside the image explicitly; only the image and channel axes, over
which every operation is elementwise, are numpy vectors.  Window (oh, ow) starts at input
pixel (oh*sh - pt, ow*sw - pl); taps outside the image do not exist.  Nothing is rounded
here: the caller applies :func:`bf16_rne` where the kernel stores bf16."""
import numpy as np

from pool_oracle import bf16_rne, same_pad  # noqa: F401  (bf16_rne: re-exported for the tests)

# (H, W) x (k, s) x padding x C of tests/test_dwconv_oracle.py (oracle against torch on the CPU)
# and tests/test_dwconv_kernels_gpu.py (kernels against the oracle)
GEOMETRIES = [((2, h, w, c), k, s, p) for (h, w) in ((9, 7), (8, 10))
              for (k, s) in ((1, 1), (3, 1), (3, 2), (5, 1), (5, 2), (7, 2)) for p in ("valid", "same")
              for c in (8, 24)]


def make_geo(shape, k, s, padding):
    """The 12-int geometry list, worked out here and not by the code under test."""
    n, h, w, c = shape
    if padding == "same":
        ho, pt = same_pad(h, k, s)
        wo, pl = same_pad(w, k, s)
    elif padding == "valid":
        ho, pt = (h - k) // s + 1, 0
        wo, pl = (w - k) // s + 1, 0
    else:
        raise ValueError(padding)
    return [n, h, w, c, k, k, s, s, pt, pl, ho, wo]


def _taps(geo):
    """(oh, i, ih, j, ows, iws): for output row oh and tap (i, j) with input row ih inside the
    image, the output columns ows whose input column iws = ow*sw - pl + j is inside it."""
    n, h, w, c, kh, kw, sh, sw, pt, pl, ho, wo = geo
    for oh in range(ho):
        for i in range(kh):
            ih = oh * sh - pt + i
            if not 0 <= ih < h:
                continue
            for j in range(kw):
                ows = [ow for ow in range(wo) if 0 <= ow * sw - pl + j < w]
                if ows:
                    yield oh, i, ih, j, ows, [ow * sw - pl + j for ow in ows]


def fwd(x, w, bias, relu, geo):
    """act(sum of the in-bounds taps + bias), unrounded."""
    n, h, wd, c, kh, kw, sh, sw, pt, pl, ho, wo = geo
    y = np.zeros((n, ho, wo, c))
    for oh, i, ih, j, ows, iws in _taps(geo):
        y[:, oh, ows, :] += x[:, ih, iws, :] * w[i, j]
    if bias is not None:
        y += bias
    return np.maximum(y, 0.0) if relu else y


def dgrad(dy, w, geo):
    n, h, wd, c, kh, kw, sh, sw, pt, pl, ho, wo = geo
    dx = np.zeros((n, h, wd, c))
    for oh, i, ih, j, ows, iws in _taps(geo):
        dx[:, ih, iws, :] += dy[:, oh, ows, :] * w[i, j]
    return dx


def wgrad(x, dy, geo):
    n, h, wd, c, kh, kw, sh, sw, pt, pl, ho, wo = geo
    dw = np.zeros((kh, kw, c))
    for oh, i, ih, j, ows, iws in _taps(geo):
        dw[i, j] += (x[:, ih, iws, :] * dy[:, oh, ows, :]).sum(axis=(0, 1))
    return dw


def bias_grad(dy):
    return dy.sum(axis=(0, 1, 2))


def ints(shape, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape).astype(np.float64)


def int_inputs(geo):
    """The integer-valued inputs of the bitwise tests: x in [-3, 3] (seed 104), w in [-2, 2]
    (105), bias in [-4, 4] (106), dy in [-4, 4] (102)."""
    n, h, w, c, kh, kw = geo[:6]
    return (ints((n, h, w, c), -3, 3, 104), ints((kh, kw, c), -2, 2, 105), ints((c,), -4, 4, 106),
            ints((n, geo[10], geo[11], c), -4, 4, 102))
