"""csrc/kernels/dwconv.hip through its launchers (ops/hip.py dwconv_fwd / dwconv_dgrad /
dwconv_wgrad) against the explicit-loop fp64 oracle of tests/helpers/dwconv_oracle.py (itself
checked against ops/reference.py and autograd in tests/test_dwconv_oracle.py).

Rectangular images, 'valid' and 'same' (pt != pb, the odd row / column below / right), kernels
1 - 7 with strides 1 / 2, one and three channel groups, and one case past the launch-grid cap.

The inputs are small integers (x in [-3, 3], w in [-2, 2], bias in [-4, 4], dy in [-4, 4]):
over these geometries max |y| = 63, max |dx| = 73, max |dw| = 175 (test_dwconv_oracle.py
prints them), so every fp32 sum is exact in any order and every bf16 store is exact -- the
comparisons are bitwise (torch.equal); each test asserts those magnitudes from the oracle.
Outputs start as NaN (dw as integers: the launch adds into it), so an element no thread wrote
shows, and at least half of every reference output is non-zero, so a kernel that writes zeros
cannot pass.  One case per kernel runs standard-normal data: two launches must agree bitwise
and stay within |got - ref| <= 2^-8 |ref| + (n + 2) 2^-24 sum|terms| of the fp64 oracle (one
bf16 rounding, dropped for the fp32 dw, plus the fp32 accumulation bound of n terms, valid for
any summation order)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dwconv_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0") if torch.cuda.is_available() else None


@pytest.fixture(scope="module")
def H():
    from distributed_amd.ops import hip

    return hip


def _ids(g):
    (n, h, w, c), k, s, p = g
    return f"{h}x{w}x{c}-k{k}s{s}-{p}"


@functools.lru_cache(maxsize=None)
def int_case(case):
    """(geo, inputs, references) of one geometry, computed once and shared by its tests."""
    shape, k, s, p = case
    geo = O.make_geo(shape, k, s, p)
    x, w, b, dy = O.int_inputs(geo)
    return tuple(geo), (x, w, b, dy), Refs({
        "y": lambda: O.fwd(x, w, None, False, geo), "y_bias_relu": lambda: O.fwd(x, w, b, True, geo),
        "y_bias": lambda: O.fwd(x, w, b, False, geo), "dx": lambda: O.dgrad(dy, w, geo),
        "dw": lambda: O.wgrad(x, dy, geo)})


class Refs(dict):
    """The oracle results of one geometry, each computed when first asked for and then kept."""

    def __init__(self, makers):
        super().__init__()
        self.makers = makers

    def __missing__(self, key):
        self[key] = self.makers[key]()
        return self[key]


def bf(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(torch.bfloat16).to(dev).contiguous()


def f32(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32).to(dev).contiguous()


def nan_bf16(shape):
    return torch.full(tuple(shape), float("nan"), dtype=torch.bfloat16, device=dev)


def check_exact(ref, bf16_out, floor=0.5):
    """The oracle's values are exactly representable (and exactly summable in fp32) and at
    least ``floor`` of them are non-zero."""
    assert np.abs(ref).max() < (256 if bf16_out else 2 ** 24)
    if bf16_out:
        assert np.array_equal(O.bf16_rne(ref), ref)
    assert (ref != 0).mean() >= floor, (ref != 0).mean()


def equal_bits(got, ref):
    want = torch.tensor(ref, dtype=torch.float32)
    got = got.float().cpu()
    assert not torch.isnan(got).any(), "an element was not written"
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"


def xshape(geo):
    return geo[0], geo[1], geo[2], geo[3]


def yshape(geo):
    return geo[0], geo[10], geo[11], geo[3]


@pytest.mark.parametrize("case", O.GEOMETRIES, ids=_ids)
def test_forward_is_bitwise_the_oracle(H, case):
    geo, (x, w, b, dy), ref = int_case(case)
    assert list(geo) == H.pool_geo(case[0], (case[1],) * 2, (case[2],) * 2, case[3])
    check_exact(ref["y"], True)
    check_exact(ref["y_bias"], True)  # (the pre-activation of the next launch)
    check_exact(ref["y_bias_relu"], True, floor=0.0)
    assert (ref["y_bias_relu"] != 0).any() and (ref["y_bias"] < 0).any()  # the ReLU cuts, and not everything
    xd, wd = bf(x), bf(w)
    y = nan_bf16(yshape(geo))
    H.dwconv_fwd(xd, wd, None, False, list(geo), y)
    equal_bits(y, ref["y"])
    y = nan_bf16(yshape(geo))
    H.dwconv_fwd(xd, wd, f32(b), True, list(geo), y)
    equal_bits(y, ref["y_bias_relu"])


@pytest.mark.parametrize("case", O.GEOMETRIES, ids=_ids)
def test_dgrad_is_bitwise_the_oracle_and_writes_every_element(H, case):
    geo, (x, w, b, dy), ref = int_case(case)
    check_exact(ref["dx"], True)
    dx = nan_bf16(xshape(geo))
    H.dwconv_dgrad(bf(dy), bf(w), list(geo), dx)
    equal_bits(dx, ref["dx"])


@pytest.mark.parametrize("case", O.GEOMETRIES, ids=_ids)
def test_wgrad_adds_the_oracle_bitwise(H, case):
    geo, (x, w, b, dy), ref = int_case(case)
    check_exact(ref["dw"], False)
    start = O.ints(ref["dw"].shape, -5, 5, 107)  # the launch adds into the gradient view
    dw = f32(start)
    ws = torch.full((H.dwconv_wgrad_workspace_elems(list(geo)),), float("nan"), device=dev)
    H.dwconv_wgrad(bf(x), bf(dy), list(geo), dw, workspace=ws)
    equal_bits(dw, start + ref["dw"])
    # bias gradient: colsum of dy, as for Conv2D
    db = torch.zeros(geo[3], device=dev)
    H.colsum(bf(dy), db)
    equal_bits(db, O.bias_grad(dy))


# one pass of a forward / backprop-input launch covers grid cap x 256 vectors of 8 channels:
# 2 x 513 x 513 pixels of 8 channels is 2050 more than that (the cap is read from the module)
GRID_CASE = ((2, 513, 513, 8), 3, 1, "same")


def test_past_the_grid_cap(H):
    from distributed_amd.native import require_C

    geo, (x, w, b, dy), ref = int_case(GRID_CASE)
    assert geo[0] * geo[10] * geo[11] * geo[3] // 8 > require_C().dwconv_grid_cap() * 256
    assert require_C().dwconv_wgrad_blocks(list(geo)) > 1
    for nm in ("y_bias_relu", "dx"):
        assert np.abs(ref[nm]).max() < 256
    assert np.abs(ref["dw"]).max() < 2 ** 24  # (sums of 526338 products of magnitude <= 12)
    xd, wd, dyd = bf(x), bf(w), bf(dy)
    y = nan_bf16(yshape(geo))
    H.dwconv_fwd(xd, wd, f32(b), True, list(geo), y)
    equal_bits(y, ref["y_bias_relu"])
    dx = nan_bf16(xshape(geo))
    H.dwconv_dgrad(dyd, wd, list(geo), dx)
    equal_bits(dx, ref["dx"])
    dw = torch.zeros(3, 3, 8, device=dev)
    H.dwconv_wgrad(xd, dyd, list(geo), dw)
    equal_bits(dw, ref["dw"])


# ---- non-integer data: run-to-run bits and the derived bound -------------------------------------
NORMAL_CASE = ((2, 9, 7, 24), 3, 2, "same")


@functools.lru_cache(maxsize=None)
def normal_case():
    geo = O.make_geo(*NORMAL_CASE)
    rng = np.random.default_rng(11)
    # what the kernels read: bf16 activations / taps / gradients, an fp32 bias
    x, w, b, dy = (rng.normal(size=a.shape) for a in O.int_inputs(geo))
    x, w, dy = O.bf16_rne(x), O.bf16_rne(w), O.bf16_rne(dy)
    b = b.astype(np.float32).astype(np.float64)
    return geo, x, w, b, dy


def within(got, ref, terms, n, bf16_out):
    got = got.float().cpu().numpy().astype(np.float64)
    bound = (2.0 ** -8 * np.abs(ref) if bf16_out else 0.0) + (n + 2) * 2.0 ** -24 * terms
    err = np.abs(got - ref)
    print(f"max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.isfinite(got).all() and (err <= bound).all()


def test_normal_data_forward(H):
    geo, x, w, b, dy = normal_case()
    outs = []
    for _ in range(2):
        y = nan_bf16(yshape(geo))
        H.dwconv_fwd(bf(x), bf(w), f32(b), False, geo, y)
        outs.append(y)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    within(outs[0], O.fwd(x, w, b, False, geo), O.fwd(np.abs(x), np.abs(w), np.abs(b), False, geo),
           geo[4] * geo[5] + 1, True)


def test_normal_data_dgrad(H):
    geo, x, w, b, dy = normal_case()
    outs = []
    for _ in range(2):
        dx = nan_bf16(xshape(geo))
        H.dwconv_dgrad(bf(dy), bf(w), geo, dx)
        outs.append(dx)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    within(outs[0], O.dgrad(dy, w, geo), O.dgrad(np.abs(dy), np.abs(w), geo), geo[4] * geo[5], True)


def test_normal_data_wgrad(H):
    geo, x, w, b, dy = normal_case()
    outs = []
    for _ in range(2):
        dw = torch.zeros(geo[4], geo[5], geo[3], device=dev)
        H.dwconv_wgrad(bf(x), bf(dy), geo, dw)
        outs.append(dw)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    within(outs[0], O.wgrad(x, dy, geo), O.wgrad(np.abs(x), np.abs(dy), geo), geo[0] * geo[10] * geo[11], False)
