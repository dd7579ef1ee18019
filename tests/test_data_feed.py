"""DataFeed's epoch-ordered copies and its bind cache (engine/data.py) on the CPU device:
what both native engines read their batches from, and the rule by which every engine
decides whether a fit brings the data it already holds."""
import numpy as np
import pytest
import torch

from distributed_amd.engine.data import DataFeed

N = 10
CPU = torch.device("cpu")


def _arrays(u8, dense, weighted):
    rng = np.random.default_rng(5)
    if u8:  # exactly k / 255: kept as uint8 rows
        x = (rng.integers(0, 256, (N, 4, 3, 1)).astype(np.uint8) / 255.0).astype(np.float32)
    else:
        x = rng.random((N, 4, 3, 1), dtype=np.float32)
    y = rng.random((N, 3), dtype=np.float32) if dense else rng.integers(0, 3, N).astype(np.int64)
    w = rng.random(N, dtype=np.float32) + 0.5 if weighted else None
    return x, y, w


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dense", [False, True], ids=["class-ids", "dense"])
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "fp32"])
def test_epoch_copies_follow_the_permutation_at_stable_addresses(u8, dense, weighted):
    x, y, w = _arrays(u8, dense, weighted)
    feed = DataFeed(x, y, CPU, flatten=True, allow_u8=True, w=w)
    assert feed.x_u8 == u8 and feed.x.dtype == (torch.uint8 if u8 else torch.float32)
    assert feed.y.dtype == (torch.float32 if dense else torch.int32)
    feed.alloc_epoch()
    assert (feed.w_ep is not None) == weighted
    copies = [t for t in (feed.x_ep, feed.y_ep, feed.w_ep) if t is not None]
    ptrs = [t.data_ptr() for t in copies]
    perms = []
    for epoch in range(3):
        feed.set_epoch(epoch, True, 11)
        feed.fill_epoch()
        perm = feed.perm.long()
        perms.append(perm.tolist())
        assert sorted(perms[-1]) == list(range(N))
        assert torch.equal(feed.x_ep, feed.x[perm]) and feed.x_ep.shape == (N, 12)
        assert torch.equal(feed.y_ep, feed.y[perm])
        if weighted:
            assert torch.equal(feed.w_ep, feed.w[perm])
            assert np.array_equal(feed.w_ep.numpy(), w[perm.numpy()])
        assert [t.data_ptr() for t in copies] == ptrs
    assert perms[0] != perms[1] and perms[1] != perms[2]  # (a real shuffle: the equalities above are not trivial)
    feed.set_epoch(3, False)
    feed.fill_epoch()
    assert torch.equal(feed.x_ep, feed.x) and torch.equal(feed.y_ep, feed.y)
    assert [t.data_ptr() for t in copies] == ptrs


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_built_from(weighted):
    x, y, w = _arrays(False, False, weighted)
    feed = DataFeed(x, y, CPU, w=w)
    assert feed.built_from(x, y, w)
    assert feed.built_from(x, y, None if w is None else w.copy())  # weights compare by value
    assert not feed.built_from(x.copy(), y, w)  # another array object
    assert not feed.built_from(x, y.copy(), w)
    assert not feed.built_from(x[:-1], y[:-1], None if w is None else w[:-1])  # another length
    xs, ys = list(x), list(y)  # the same objects at another length
    grown = DataFeed(xs, ys, CPU)
    assert grown.built_from(xs, ys)
    xs.pop(), ys.pop()
    assert not grown.built_from(xs, ys)
    if weighted:
        assert not feed.built_from(x, y, None)  # weights removed
        w2 = w.copy()
        w2[3] += 0.25
        assert not feed.built_from(x, y, w2)  # one element changed
    else:
        assert not feed.built_from(x, y, np.ones(N, dtype=np.float32))  # weights added
