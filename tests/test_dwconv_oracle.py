"""The fp64 oracle of tests/helpers/dwconv_oracle.py against ops/reference.py
depthwise_conv2d (the definition) and autograd, in fp64 on the CPU, on every geometry the GPU
kernel tests use -- and the facts about the integer data those tests lean on: every value
stays small enough for exact fp32 sums and exact bf16 stores, and most outputs are non-zero."""
import os
import sys

import numpy as np
import pytest
import torch

from distributed_amd.ops import hip as H
from distributed_amd.ops import reference

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dwconv_oracle as O  # noqa: E402


def _ids(g):
    (n, h, w, c), k, s, p = g
    return f"{h}x{w}x{c}-k{k}s{s}-{p}"


@pytest.mark.parametrize("case", O.GEOMETRIES, ids=_ids)
def test_geometry_is_pool_geo(case):
    shape, k, s, p = case
    assert O.make_geo(shape, k, s, p) == H.pool_geo(shape, (k, k), (s, s), p)


@pytest.mark.parametrize("case", O.GEOMETRIES, ids=_ids)
@pytest.mark.parametrize("data", ["int", "normal"])
def test_oracle_matches_reference_and_autograd(case, data):
    shape, k, s, p = case
    geo = O.make_geo(shape, k, s, p)
    if data == "int":
        x, w, b, dy = O.int_inputs(geo)
    else:
        rng = np.random.default_rng(7)
        x, w, b, dy = (rng.normal(size=a.shape) for a in O.int_inputs(geo))
    xt, wt, bt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, w, b))
    for relu in (False, True):
        y = reference.depthwise_conv2d(xt, wt[..., None], bt, (s, s), p)
        y = torch.relu(y) if relu else y
        assert tuple(y.shape) == (geo[0], geo[10], geo[11], geo[3])
        np.testing.assert_allclose(O.fwd(x, w, b, relu, geo), y.detach().numpy(), rtol=1e-12, atol=1e-12)
    y = reference.depthwise_conv2d(xt, wt[..., None], bt, (s, s), p)
    gx, gw, gb = torch.autograd.grad(y, (xt, wt, bt), torch.tensor(dy))
    np.testing.assert_allclose(O.dgrad(dy, w, geo), gx.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(O.wgrad(x, dy, geo), gw.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(O.bias_grad(dy), gb.numpy(), rtol=1e-12, atol=1e-12)
    # no bias
    y0 = reference.depthwise_conv2d(xt, wt[..., None], None, (s, s), p)
    np.testing.assert_allclose(O.fwd(x, w, None, False, geo), y0.detach().numpy(), rtol=1e-12, atol=1e-12)


def test_integer_data_is_exact_and_not_vacuous():
    """What makes the GPU tests' bitwise comparison valid, over all of their geometries."""
    ymax = dxmax = dwmax = 0.0
    share = {"y": 1.0, "dx": 1.0, "dw": 1.0}
    for shape, k, s, p in O.GEOMETRIES:
        geo = O.make_geo(shape, k, s, p)
        x, w, b, dy = O.int_inputs(geo)
        outs = {"y": O.fwd(x, w, b, False, geo), "dx": O.dgrad(dy, w, geo), "dw": O.wgrad(x, dy, geo)}
        ymax = max(ymax, np.abs(outs["y"]).max(), np.abs(O.fwd(x, w, None, False, geo)).max())
        dxmax, dwmax = max(dxmax, np.abs(outs["dx"]).max()), max(dwmax, np.abs(outs["dw"]).max())
        for nm, a in outs.items():
            share[nm] = min(share[nm], float((a != 0).mean()))
    print(f"max |y| {ymax}, max |dx| {dxmax}, max |dw| {dwmax}, non-zero shares {share}")
    assert ymax < 256 and dxmax < 256 and dwmax < 2 ** 24
    assert min(share.values()) >= 0.5, share
