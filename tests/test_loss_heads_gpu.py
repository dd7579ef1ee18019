"""The dense-target loss kernel (softmax_xent_dense_k) and the probability predict tail
(softmax_store_k) against the fp32 oracles of distributed_amd/ops/reference.py.

Shapes: the padded 10-class head, the register path's limit (1024 = 4 x 256 values per
row), the ResNet-18 head (64 x 1000) and a row the kernels re-read (1500).  Tolerances are
the ones test_hip_ops_gpu.py uses for the sparse kernel: bf16 gradients (1e-2, 4e-3), fp32
sums (1e-5, 1e-6), fp32 outputs (1e-4, 1e-5)."""
import pytest
import torch

from distributed_amd.engine.ctrl import C_CUR, C_GB, C_NS, C_ROW0, C_WRAP
from distributed_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

dev = torch.device("cuda:0") if torch.cuda.is_available() else None

SHAPES = [(5, 10, 16), (7, 1024, 1024), (64, 1000, 1000), (3, 1500, 1504)]


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


def _onehot(n, K, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, K, (n,), generator=g)
    return torch.nn.functional.one_hot(ids, K).float().to(dev), ids.to(dev)


def _case(kind, B, K, ld, seed=40):
    """(logits [B, ld], targets [B, K]) for one kind of target row."""
    z = rnd(B, ld, seed=seed)
    if kind in ("onehot", "twice"):
        y, ids = _onehot(B, K, seed + 1)
        rows = torch.arange(0, B, 2, device=dev)
        z[rows, ids[rows]] += 10.0  # every other row is classified correctly
        if kind == "twice":
            y = 2.0 * y  # the targets of a row sum to 2, not 1
    else:
        y = torch.softmax(rnd(B, K, seed=seed + 2), -1)
        if kind == "tie":
            # a tie for the max at the same two columns of the logits and the targets: both
            # argmaxes go to the smaller index, so row 0 counts as correct
            z[0, 5] = z[0, 9] = z[0, :K].max() + 1.0
            y[0, 5] = y[0, 9] = y[0].max() * 1.5
    return z, y.contiguous()


def _reference(z, y, K, eps, scale):
    zz = z[:, :K].clone().requires_grad_(True)
    loss = ref.softmax_xent_dense(zz, y, eps)
    (gz,) = torch.autograd.grad(loss.sum() * scale, (zz,))
    return loss.detach(), gz


@pytest.mark.parametrize("kind", ["onehot", "soft", "twice", "tie"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,K,ld", SHAPES)
def test_softmax_xent_dense(H, B, K, ld, eps, kind):
    z, y = _case(kind, B, K, ld)
    dl = torch.ones(B, ld, device=dev, dtype=torch.bfloat16)
    tail = torch.zeros(3, device=dev)
    H.softmax_xent_dense(z, y, K, 1.0 / B, dl, tail, label_smoothing=eps)
    loss, gz = _reference(z, y, K, eps, 1.0 / B)
    close(dl[:, :K], gz, 1e-2, 4e-3)
    assert ld == K or torch.all(dl[:, K:] == 1).item()  # pad columns are never written
    close(tail[0], loss.sum(), 1e-5, 1e-6)
    correct = ref.categorical_accuracy(z[:, :K], y).sum().item()
    assert tail[1].item() == correct
    if kind in ("onehot", "twice"):
        assert correct >= (B + 1) // 2
    if kind == "tie":
        assert y[0].argmax().item() == 5 and z[0, :K].argmax().item() == 5 and correct >= 1
    assert tail[2].item() == B
    # a second run gives the same bits (fixed-order sums, no float atomics)
    dl2 = torch.ones_like(dl)
    tail2 = torch.zeros(3, device=dev)
    H.softmax_xent_dense(z, y, K, 1.0 / B, dl2, tail2, label_smoothing=eps)
    assert torch.equal(dl, dl2) and torch.equal(tail, tail2)
    # the bias-gradient fold adds exactly what colsum adds
    if H.softmax_bias_fold_ok(B, K):
        base = rnd(K, seed=32)
        bg, bc = base.clone(), base.clone()
        dl3 = torch.zeros_like(dl)
        H.softmax_xent_dense(z, y, K, 1.0 / B, dl3, torch.zeros(3, device=dev), label_smoothing=eps, bias_grad=bg)
        H.colsum(dl3, bc, M=B, N=K, ld=ld)
        assert torch.equal(bg, bc)
        assert torch.equal(dl3[:, :K], dl[:, :K])


def test_one_hot_rows_give_the_sparse_kernel_result(H):
    """eps = 0 and one-hot rows: S = 1 and the dot product is the label's logit, so the
    dense kernel agrees with softmax_xent_k on the gradient bits and, to fp32 rounding, on
    the loss."""
    B, K, ld = 64, 1000, 1000
    z, y = _case("onehot", B, K, ld)
    lab = y.argmax(-1).to(torch.int32)
    dl, dls = (torch.zeros(B, ld, device=dev, dtype=torch.bfloat16) for _ in range(2))
    tail, tails = torch.zeros(3, device=dev), torch.zeros(3, device=dev)
    H.softmax_xent_dense(z, y, K, 1.0 / B, dl, tail)
    H.softmax_xent(z, lab, K, 1.0 / B, dls, tails)
    assert torch.equal(dl, dls)
    close(tail[0], tails[0], 1e-6, 0.0)
    assert torch.equal(tail[1:], tails[1:])


@pytest.mark.parametrize("K,ld", [(10, 16), (1000, 1000), (1500, 1504)])
def test_dense_targets_are_read_at_the_device_cursor(H, K, ld):
    """With the control block the kernel finds its target rows itself, as gather_batch finds
    the input rows: row cursor * global_batch + row0 + b (modulo nsamples in wrap mode);
    labels < 0 (rows past the end of the data) give a zero gradient and no loss, metric or
    count; the scale is 1 / (rows of this global batch that exist)."""
    B, n, gb, row0, cursor = 4, 11, 8, 4, 1
    base = cursor * gb + row0  # 12: rows 8..10 of this global batch exist, 3 of 8
    z = rnd(B, ld, seed=50)
    y, _ = _onehot(16, K, seed=51)
    y = (0.7 * y + 0.3 * torch.softmax(rnd(16, K, seed=52), -1)).contiguous()  # 16 distinct rows
    lab = torch.tensor([0, -1, 0, -1], device=dev, dtype=torch.int32)
    keep = torch.tensor([0, 2], device=dev)
    dl = torch.ones(B, ld, device=dev, dtype=torch.bfloat16)
    tail = torch.zeros(3, device=dev)
    H.softmax_xent_dense(z, y, K, 123.0, dl, tail, label_smoothing=0.1, labels=lab, ctrl=_ctrl(n, gb, row0, cursor))
    loss, gz = _reference(z, y[base:base + B], K, 0.1, 1.0 / 3.0)
    close(dl[keep, :K], gz[keep], 1e-2, 4e-3)
    assert dl[1, :K].abs().max().item() == 0 and dl[3, :K].abs().max().item() == 0
    assert ld == K or torch.all(dl[:, K:] == 1).item()
    close(tail[0], loss[keep].sum(), 1e-5, 1e-6)
    assert tail[1].item() == ref.categorical_accuracy(z[keep, :K], y[base:base + B][keep]).sum().item()
    assert tail[2].item() == 2
    # wrap mode (benchmark epochs): every row is real, rows (base + b) % n, scale 1 / global batch
    lab0 = torch.zeros(B, device=dev, dtype=torch.int32)
    dlw = torch.ones(B, ld, device=dev, dtype=torch.bfloat16)
    tailw = torch.zeros(3, device=dev)
    H.softmax_xent_dense(z, y, K, 123.0, dlw, tailw, label_smoothing=0.1, labels=lab0,
                         ctrl=_ctrl(n, gb, row0, cursor, wrap=5))
    rows = (base + torch.arange(B, device=dev)) % n  # 1, 2, 3, 4
    lossw, gzw = _reference(z, y[rows], K, 0.1, 1.0 / gb)
    close(dlw[:, :K], gzw, 1e-2, 4e-3)
    close(tailw[0], lossw.sum(), 1e-5, 1e-6)
    assert tailw[2].item() == B


def test_launcher_checks(H):
    z = rnd(4, 16, seed=60)
    dl = torch.zeros(4, 16, device=dev, dtype=torch.bfloat16)
    tail = torch.zeros(3, device=dev)
    y = torch.zeros(4, 10, device=dev)
    with pytest.raises(ValueError):
        H.softmax_xent_dense(z, torch.zeros(4, 12, device=dev), 10, 1.0, dl, tail)  # not K wide
    with pytest.raises(TypeError):
        H.softmax_xent_dense(z, y.double(), 10, 1.0, dl, tail)
    with pytest.raises(ValueError):
        H.softmax_xent_dense(z, torch.zeros(10, 4, device=dev).t(), 10, 1.0, dl, tail)  # not contiguous
    with pytest.raises(ValueError):
        H.softmax_xent_dense(z, y, 10, 1.0, dl, tail, label_smoothing=1.0)
    with pytest.raises(ValueError):
        H.softmax_xent_dense(z, y[:3], 10, 1.0, dl, tail)  # fewer target rows than logits rows
    with pytest.raises(ValueError):
        H.softmax_xent_dense(z, y, 10, 1.0, dl, tail, ctrl=_ctrl(4, 4, 0, 0))  # ctrl without labels
    with pytest.raises(ValueError):
        H.softmax_store(z, 10, _ctrl(4, 4, 0, 0), torch.zeros(4, 12, device=dev))


@pytest.mark.parametrize("B,K,ld", SHAPES)
def test_softmax_store(H, B, K, ld):
    """Rows of step ``cursor`` land at their global row as probabilities; the rows of the
    short last batch that do not exist are dropped, nothing else is touched."""
    n = 2 * B - 2  # step 1 holds rows B .. 2B - 1: its last two are past the end
    z = rnd(B, ld, seed=70)
    z[0, :K] *= 8.0  # a peaked row
    out = torch.full((2 * B, K), -1.0, device=dev)
    H.softmax_store(z, K, _ctrl(n, B, 0, 1), out)
    p = torch.softmax(z[:B - 2, :K], -1)
    close(out[B:n], p, 1e-4, 1e-5)
    assert (out[B:n].sum(-1) - 1.0).abs().max().item() < 1e-5
    assert torch.all(out[:B] == -1).item() and torch.all(out[n:] == -1).item()
