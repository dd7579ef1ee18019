"""Per-row weights in the two loss kernels (softmax_xent_k<true>, softmax_xent_dense_k<true>)
against the fp32 oracles of distributed_amd/ops/reference.py: a row's gradient and loss are
multiplied by its weight, the correct / valid counts are not.

Shapes: the padded 10-class head, the register path's limit (1024 = 4 x 256 values per row)
and a row the kernels re-read (1500).  Tolerances are the ones test_loss_heads_gpu.py states
for these kernels: bf16 gradients (1e-2, 4e-3), fp32 sums (1e-5, 1e-6)."""
import pytest
import torch

from distributed_amd.engine.ctrl import C_CUR, C_GB, C_NS, C_ROW0, C_WRAP
from distributed_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0") if torch.cuda.is_available() else None

SHAPES = [(5, 10, 16), (7, 1024, 1024), (3, 1500, 1504)]
KINDS = ["sparse", "dense"]
WEIGHTS = [0.0, 0.25, 1.0, 3.5, 0.5, 2.0, 1.5]  # distinct per row; row 0 has weight 0
EPS = 0.1  # the dense kernel's label smoothing


@pytest.fixture(scope="module")
def H():
    from distributed_amd.ops import hip

    return hip


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def close(a, b, rtol, atol_frac):
    a, b = a.float(), b.float()
    atol = atol_frac * b.abs().max().item() + 1e-12
    err = (a - b).abs().max().item()
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"max abs err {err:.3e} (atol {atol:.3e})"


def _ctrl(nsamples, global_batch, row0, cursor, wrap=0):
    c = torch.zeros(32, dtype=torch.int32)
    c[C_NS], c[C_GB], c[C_ROW0], c[C_CUR], c[C_WRAP] = nsamples, global_batch, row0, cursor, wrap
    return c.to(dev)


def _targets(n, K, seed):
    """(class ids [n], soft target rows [n, K] whose argmax is the id)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, K, (n,), generator=g).to(dev)
    y = 0.7 * torch.nn.functional.one_hot(ids, K).float() + 0.3 * torch.softmax(rnd(n, K, seed=seed + 1), -1)
    return ids, y.contiguous()


def _launch(H, kind, z, ids, y, K, scale, dl, tail, **kw):
    if kind == "sparse":
        lab = kw.pop("labels", None)
        H.softmax_xent(z, ids.to(torch.int32) if lab is None else lab, K, scale, dl, tail, **kw)
    else:
        H.softmax_xent_dense(z, y, K, scale, dl, tail, label_smoothing=EPS, **kw)


def _oracle(kind, z, ids, y, K, w, scale):
    """(weighted per-row loss, gradient of sum(w * loss) * scale, per-row correct)."""
    zz = z[:, :K].clone().requires_grad_(True)
    if kind == "sparse":
        loss = ref.sparse_softmax_xent(zz, ids, weights=w)
        corr = ref.sparse_accuracy(z[:, :K], ids)
    else:
        loss = ref.softmax_xent_dense(zz, y, EPS, weights=w)
        corr = ref.categorical_accuracy(z[:, :K], y)
    (gz,) = torch.autograd.grad(loss.sum() * scale, (zz,))
    return loss.detach(), gz, corr


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,K,ld", SHAPES)
def test_weighted_loss_kernels(H, B, K, ld, kind):
    z = rnd(B, ld, seed=40)
    ids, y = _targets(B, K, seed=41)
    rows = torch.arange(0, B, 2, device=dev)
    z[rows, ids[rows]] += 10.0  # every other row is classified correctly
    w = torch.tensor(WEIGHTS[:B], device=dev)
    dl = torch.ones(B, ld, device=dev, dtype=torch.bfloat16)
    tail = torch.zeros(3, device=dev)
    _launch(H, kind, z, ids, y, K, 1.0 / B, dl, tail, weights=w)
    loss, gz, corr = _oracle(kind, z, ids, y, K, w, 1.0 / B)
    close(dl[:, :K], gz, 1e-2, 4e-3)
    close(tail[0], loss.sum(), 1e-5, 1e-6)
    # the counts are unweighted: the weight-0 row still counts, and is classified correctly
    assert tail[1].item() == corr.sum().item() and corr[0].item() == 1 and corr.sum().item() >= (B + 1) // 2
    assert tail[2].item() == B
    assert dl[0, :K].abs().max().item() == 0  # weight 0: exactly zero
    assert dl[1, :K].abs().max().item() > 0
    assert ld == K or torch.all(dl[:, K:] == 1).item()  # pad columns are never written
    # the unweighted launch on the same inputs: the same counts, another loss
    dlu = torch.ones_like(dl)
    tailu = torch.zeros(3, device=dev)
    _launch(H, kind, z, ids, y, K, 1.0 / B, dlu, tailu)
    assert torch.equal(tailu[1:], tail[1:]) and tailu[0].item() != tail[0].item()
    # a second run gives the same bits (fixed-order sums, no float atomics)
    dl2 = torch.ones_like(dl)
    tail2 = torch.zeros(3, device=dev)
    _launch(H, kind, z, ids, y, K, 1.0 / B, dl2, tail2, weights=w)
    assert torch.equal(dl, dl2) and torch.equal(tail, tail2)
    # all-ones weights: the unweighted kernel's bits
    dl1 = torch.ones_like(dl)
    tail1 = torch.zeros(3, device=dev)
    _launch(H, kind, z, ids, y, K, 1.0 / B, dl1, tail1, weights=torch.ones(B, device=dev))
    assert torch.equal(dl1, dlu) and torch.equal(tail1, tailu)
    # the bias-gradient fold adds exactly the column sums of the weighted dl
    if H.softmax_bias_fold_ok(B, K):
        base = rnd(K, seed=32)
        bg, bc = base.clone(), base.clone()
        dl3 = torch.zeros_like(dl)
        _launch(H, kind, z, ids, y, K, 1.0 / B, dl3, torch.zeros(3, device=dev), weights=w, bias_grad=bg)
        H.colsum(dl3, bc, M=B, N=K, ld=ld)
        assert torch.equal(bg, bc)
        assert torch.equal(dl3[:, :K], dl[:, :K])
        assert not torch.equal(bg, base)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,ld", [(10, 16), (1500, 1504)])
def test_weights_are_read_at_the_device_cursor(H, K, ld, kind):
    """With the control block the weight of logits row b is the weight of sample cursor *
    global_batch + row0 + b (modulo nsamples in wrap mode): the row softmax_xent_dense_k
    takes its targets from.  A row with label < 0 never reads the array.

    B = 4, n = 11, global batch 8, row0 = 4, cursor 1 (three of the eight rows exist, scale
    1/3), labels [0, -1, 0, -1].  As in test_loss_heads_gpu.py's cursor test the kernel then
    addresses rows 12 .. 15, past nsamples, so the arrays the cursor walks hold 16 distinct
    entries; the weights continue with NaN padding, and the entries of the two label < 0 rows
    (13, 15) are NaN as well: a read of either shows as a NaN tail.  In wrap mode the rows are
    (12 + b) % 11 = 1 .. 4 of an array of n = 11 distinct weights followed by NaN padding."""
    B, n, gb, row0, cursor = 4, 11, 8, 4, 1
    base = cursor * gb + row0  # 12
    z = rnd(B, ld, seed=50)
    ids, y = _targets(16, K, seed=51)
    ids[:] = 0  # the sparse kernel's labels are the step's: class 0 for a real row
    lab = torch.tensor([0, -1, 0, -1], device=dev, dtype=torch.int32)
    keep = torch.tensor([0, 2], device=dev)
    nan = float("nan")
    w = torch.cat([0.5 + 0.25 * torch.arange(16), torch.full((16,), nan)]).to(dev)
    w[base + 1] = w[base + 3] = nan
    dl = torch.ones(B, ld, device=dev, dtype=torch.bfloat16)
    tail = torch.zeros(3, device=dev)
    _launch(H, kind, z, ids, y, K, 123.0, dl, tail, labels=lab, ctrl=_ctrl(n, gb, row0, cursor), weights=w)
    wk = torch.nan_to_num(w[base:base + B])  # (rows 1 and 3 are dropped below)
    loss, gz, corr = _oracle(kind, z, ids[base:base + B], y[base:base + B], K, wk, 1.0 / 3.0)
    close(dl[keep, :K], gz[keep], 1e-2, 4e-3)
    assert dl[1, :K].abs().max().item() == 0 and dl[3, :K].abs().max().item() == 0
    assert ld == K or torch.all(dl[:, K:] == 1).item()
    assert torch.isfinite(tail).all().item()
    close(tail[0], loss[keep].sum(), 1e-5, 1e-6)
    assert tail[1].item() == corr[keep].sum().item()
    assert tail[2].item() == 2
    # wrap mode (benchmark epochs): every row is real, rows (base + b) % n, scale 1 / global batch
    lab0 = torch.zeros(B, device=dev, dtype=torch.int32)
    ww = torch.cat([3.0 - 0.25 * torch.arange(n), torch.full((21,), nan)]).to(dev)
    dlw = torch.ones(B, ld, device=dev, dtype=torch.bfloat16)
    tailw = torch.zeros(3, device=dev)
    _launch(H, kind, z, ids, y, K, 123.0, dlw, tailw, labels=lab0, ctrl=_ctrl(n, gb, row0, cursor, wrap=5),
            weights=ww)
    rows = (base + torch.arange(B, device=dev)) % n  # 1, 2, 3, 4
    lossw, gzw, corrw = _oracle(kind, z, ids[rows], y[rows], K, ww[rows], 1.0 / gb)
    close(dlw[:, :K], gzw, 1e-2, 4e-3)
    assert torch.isfinite(tailw).all().item()
    close(tailw[0], lossw.sum(), 1e-5, 1e-6)
    assert tailw[1].item() == corrw.sum().item()
    assert tailw[2].item() == B


def test_launcher_checks(H):
    z = rnd(4, 16, seed=60)
    dl = torch.zeros(4, 16, device=dev, dtype=torch.bfloat16)
    tail = torch.zeros(3, device=dev)
    lab = torch.zeros(4, device=dev, dtype=torch.int32)
    y = torch.zeros(4, 10, device=dev)
    w = torch.ones(8, device=dev)
    for run in (lambda **kw: H.softmax_xent(z, lab, 10, 1.0, dl, tail, **kw),
                lambda **kw: H.softmax_xent_dense(z, y, 10, 1.0, dl, tail, **kw)):
        with pytest.raises(ValueError):
            run(weights=w.double())  # fp64
        with pytest.raises(ValueError):
            run(weights=w[::2])  # not contiguous
        with pytest.raises(ValueError):
            run(weights=w[:3])  # fewer than B without ctrl
        with pytest.raises(ValueError):
            run(weights=torch.ones(4, 1, device=dev))  # not 1-D
        run(weights=w[:4])
