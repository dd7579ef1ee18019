"""Gradient clipping on the GPU: the grad_norm reduction and the opt_step kernel's clip
modes against the fp64 / fp32 host reference, and whole native-engine runs (closed form of
one step, the generic engine, graph replay, per-bucket updates, BatchNorm variables)."""
import math

import numpy as np
import pytest
import torch

import distributed_amd as tf
from distributed_amd.engine.ctrl import C_CUR3, C_IT
from distributed_amd.ops import hip as H
from distributed_amd.ops import reference as R

import test_regularizers_gpu as TR
from test_native_graph_gpu import _data, _mnist, _train

pytestmark = pytest.mark.gpu
dev = "cuda"
O = tf.keras.optimizers
MODES = ("clipvalue", "clipnorm", "global_clipnorm")

# test_regularizers_gpu's layout (padding gaps, a variable shorter than one vector, 4099 =
# one whole chunk + 3 elements, in two blocks) and one variable of three chunks;
# (l1 only), (no row), (l2 only), (both), (no row), (l2 only)
SIZES = TR.SIZES + (10000,)
COEF = TR.COEF + ((0.0, 0.1),)
ZERO_VAR = 1  # this variable's gradient is all zeros (and it carries no regularizer)


def _case(reg, seed=5, scale=1.0):
    """(offsets, n, variable rows with coefficients, regularizer rows, gradient, masters)."""
    offs, n, rows = TR._layout(SIZES, COEF)
    if not reg:
        rows = []
    co = {r[0]: (r[2], r[3]) for r in rows}
    vrows = [(o, sz) + co.get(o, (0.0, 0.0)) for o, sz in zip(offs, SIZES)]
    g = TR._flat(seed, offs, n, SIZES, scale=scale)
    g[offs[ZERO_VAR]:offs[ZERO_VAR] + SIZES[ZERO_VAR]] = 0.0
    p = TR._flat(seed + 1, offs, n, SIZES, scale=0.5)
    return offs, n, vrows, rows, g, p


def _host(g, p, vrows, rows, mode, c):
    """fp64 norms and fp32 scales of the reference over g + dR/dw."""
    gh = g + R.reg_grad(p, rows) if rows else g.clone()
    return R.clip_grad(gh, vrows, mode, c)


def test_chunk_layout():
    assert H.GN_CHUNK == 4096  # SIZES' 4099 and 10000 are picked against it
    _, n, vrows, _, _, _ = _case(True)
    plan = H.clip_plan(vrows, n, dev, per_variable=True)
    assert plan.nchunk == 1 + 1 + 1 + 1 + 2 + 3 and plan.nvar == 6
    assert plan.vfirst.tolist() == [0, 1, 2, 3, 4, 6, 9]
    ct = plan.ct.tolist()
    assert ct[4] == [vrows[4][0], 4] and ct[5] == [vrows[4][0] + 4096, 4] and ct[8] == [vrows[5][0] + 8192, 5]
    with pytest.raises(ValueError):
        H.clip_plan([(4, 8)], 16, dev, True)  # not on an 8-element boundary
    with pytest.raises(ValueError):
        H.clip_plan([(0, 16), (8, 8)], 32, dev, False)  # overlap
    with pytest.raises(ValueError):
        H.clip_plan([(0, 17)], 16, dev, False)  # past the buffer
    with pytest.raises(ValueError):
        H.clip_plan([(8 * i, 8) for i in range(H.REG_MAX_ROWS + 1)], 8 * (H.REG_MAX_ROWS + 1), dev, True)
    assert H.clip_plan([(8 * i, 8) for i in range(H.REG_MAX_ROWS + 1)], 8 * (H.REG_MAX_ROWS + 1), dev, False).nout == 1


@pytest.mark.parametrize("reg", [False, True], ids=["plain", "reg"])
@pytest.mark.parametrize("mode", ["clipnorm", "global_clipnorm"])
def test_grad_norm(mode, reg):
    """Norms and scales against the fp64 host value (rtol 1e-5, reg_penalty's tolerance: a
    thread adds 16 fp32 squares, the trees and the chunk sums add ~12 levels), the re-armed
    counter, bitwise repeatability, scales of exactly 1, and a NaN scale for an inf."""
    offs, n, vrows, rows, g, p = _case(reg)
    pv = mode == "clipnorm"
    plan = H.clip_plan(vrows, n, dev, per_variable=pv)
    assert plan.regularized == reg
    G = torch.cat([g, torch.full((8,), 1e30)]).to(dev)[:n + 8]  # a metric tail behind G: never read
    P = p.to(dev) if reg else None
    n0, _ = _host(g, p, vrows, rows, mode, 1.0)
    c = float(np.median(n0)) if pv else 0.5 * n0[0]
    norms, scales = _host(g, p, vrows, rows, mode, c)
    H.grad_norm(G, plan, c, P=P)
    torch.cuda.synchronize()
    got_n, got_s = plan.norms.cpu().numpy(), plan.scales.cpu().numpy()
    print(mode, "reg" if reg else "plain", "norms", got_n, "want", norms, "scales", got_s, "want", scales)
    np.testing.assert_allclose(got_n, norms, rtol=1e-5)
    np.testing.assert_allclose(got_s, scales, rtol=1e-5)
    if pv:
        assert got_n[ZERO_VAR] == 0.0 and got_s[ZERO_VAR] == 1.0  # the zero gradient: scale 1, no 0/0
        assert (got_s == 1.0).any() and (got_s < 1.0).any()
        assert all(s == 1.0 for s, w in zip(got_s, norms) if w < c * (1 - 1e-5))
    else:
        assert got_s[0] < 1.0
    assert int(plan.scratch[-1:].view(torch.int32)) == 0  # the arrival counter re-armed
    first = plan.out.clone()
    H.grad_norm(G, plan, c, P=P)  # the same scratch: the same bits
    torch.cuda.synchronize()
    assert first.cpu().numpy().tobytes() == plan.out.cpu().numpy().tobytes()
    # c above every norm: every scale is exactly 1.0
    H.grad_norm(G, plan, 2.0 * max(norms) + 1.0, P=P)
    torch.cuda.synchronize()
    assert (plan.scales == 1.0).all()
    np.testing.assert_array_equal(plan.norms.cpu().numpy(), first[0].cpu().numpy())
    # one inf in G is data: its variable's (or the global) scale is NaN, nothing else changes
    bad = G.clone()
    bad[offs[3] + 17] = float("inf")
    H.grad_norm(bad, plan, c, P=P)
    torch.cuda.synchronize()
    s = plan.scales.cpu().numpy()
    if pv:
        assert math.isnan(s[3]) and np.array_equal(np.delete(s, 3), np.delete(first[1].cpu().numpy(), 3))
    else:
        assert math.isnan(s[0])
    assert int(plan.scratch[-1:].view(torch.int32)) == 0
    with pytest.raises(ValueError):
        H.grad_norm(G, plan, 0.0, P=P)
    if reg:
        with pytest.raises(ValueError):
            H.grad_norm(G, plan, c)  # a plan with coefficients needs the masters


class _Flat(TR._Flat):
    """test_regularizers_gpu's opt_step state with the clipping arguments."""

    def step(self, t, g, table=None, splits=None, **clip):
        self.ctrl[C_CUR3] = t
        G = g.to(dev)
        cuts = [0] + list(splits or []) + [self.n]
        for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            kw = dict(clip)
            if table is not None:
                kw.update(reg=table.data_ptr(), nreg=table.shape[0], lo=lo)
            self.C.opt_step(self.P.data_ptr() + 4 * lo, G.data_ptr() + 4 * lo, *(s.data_ptr() + 4 * lo for s in self.S),
                            self.Pb.data_ptr() + 2 * lo, hi - lo, self.ctrl.data_ptr(), self.tail.data_ptr(), self.kind,
                            *map(float, self.args[:5]), self.args[5], torch.cuda.current_stream().cuda_stream,
                            book=int(k == len(cuts) - 2), **kw)
        torch.cuda.synchronize()


# c of each mode: the steps alternate gradients of scale 0.1 and 1.0 (variable norms about
# 0.1 sqrt(size) and sqrt(size), sizes 1 .. 10000), so each c clips some and leaves some
CLIP_C = {"clipvalue": 0.5, "clipnorm": 3.0, "global_clipnorm": 40.0}


@pytest.mark.parametrize("reg", [False, True], ids=["plain", "reg"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(TR._opt_cases()))
def test_opt_step_clip_modes_match_reference(name, mode, reg):
    """grad_norm + opt_step against reg_grad + clip_grad + the Keras optimizer's own fp32
    apply_flat on the CPU, three steps (test_opt_step_with_table_matches_reference's
    tolerances); under clipvalue several launches with lo offsets == the single launch."""
    offs, n, vrows, rows, _, _ = _case(reg)
    c = CLIP_C[mode]
    plan = H.clip_plan(vrows, n, dev, per_variable=mode == "clipnorm") if mode != "clipvalue" else None
    table = plan.vt if mode == "clipnorm" else (H.reg_table(rows, dev) if rows else None)
    p0 = TR._flat(1, offs, n, SIZES)
    opt_h = TR._opt_cases()[name]()
    opt_h.ensure_slots(n, torch.device("cpu"))
    ph = p0.clone()
    one, two = _Flat(p0, TR._opt_cases()[name]()), _Flat(p0, TR._opt_cases()[name]())
    seen = set()
    for t in range(1, 4):
        g = TR._flat(10 + t, offs, n, SIZES, scale=0.1 if t % 2 else 1.0, zeros=False)
        g[offs[ZERO_VAR]:offs[ZERO_VAR] + SIZES[ZERO_VAR]] = 0.0
        kw = dict(clip=H.CLIP_KINDS[mode], clipc=c)
        if plan is not None:
            H.grad_norm(g.to(dev), plan, c, P=one.P if reg else None)
            kw["scales"] = plan.scales.data_ptr()
        one.step(t, g, table, **kw)
        gh = g + R.reg_grad(ph, rows) if rows else g.clone()
        before = gh.clone()
        _, scales = R.clip_grad(gh, vrows, mode, c)
        seen |= {bool(s < 1.0) for s in scales} if scales else set((gh != before).unique().tolist())
        opt_h.apply_flat(ph, gh)
        torch.testing.assert_close(one.P.cpu(), ph, rtol=1e-5, atol=1e-6)
        assert int(one.ctrl[C_IT]) == t
        for i, nm in enumerate(one.names):
            if nm:
                torch.testing.assert_close(one.S[i].cpu(), opt_h.slots[nm], rtol=1e-5, atol=1e-7)
        if mode == "clipvalue":  # per-bucket launches: pointers advanced, absolute lo passed
            two.step(t, g, table, splits=[offs[2], offs[4], offs[5] + 4096], **kw)
            for a, b in zip(one.state(), two.state()):
                assert a.tobytes() == b.tobytes()
    assert seen == {True, False}  # some variables / elements were clipped, some left alone
    assert torch.equal(one.Pb, one.P.bfloat16())


@pytest.mark.parametrize("mode", MODES)
def test_opt_step_scale_one_is_the_plain_launch(mode):
    """A clip that never bites leaves the bits of the launch without it (with the table)."""
    offs, n, vrows, rows, _, _ = _case(True)
    plan = H.clip_plan(vrows, n, dev, per_variable=mode == "clipnorm") if mode != "clipvalue" else None
    table = H.reg_table(rows, dev)
    p0 = TR._flat(1, offs, n, SIZES)
    a, b = _Flat(p0, O.SGD(0.05, momentum=0.9)), _Flat(p0, O.SGD(0.05, momentum=0.9))
    for t in range(1, 3):
        g = TR._flat(30 + t, offs, n, SIZES, zeros=False)
        kw = dict(clip=H.CLIP_KINDS[mode], clipc=1e6)
        if plan is not None:
            H.grad_norm(g.to(dev), plan, 1e6, P=a.P)
            kw["scales"] = plan.scales.data_ptr()
        a.step(t, g, plan.vt if mode == "clipnorm" else table, **kw)
        b.step(t, g, table)
    for x, y in zip(a.state(), b.state()):
        np.testing.assert_array_equal(x, y)


def test_opt_step_rejects_bad_clip_arguments():
    offs, n, vrows, rows, _, _ = _case(False)
    f = _Flat(TR._flat(1, offs, n, SIZES), O.SGD(0.05))
    g = TR._flat(2, offs, n, SIZES)
    for kw in (dict(clip=4), dict(clip=1, clipc=0.0), dict(clip=3), dict(clip=2, scales=f.tail.data_ptr())):
        with pytest.raises(RuntimeError):
            f.step(1, g, None, **kw)


# --- the native engine end to end ---------------------------------------------------------------
LR = 0.05
STRICT = {"DAMD_STRICT_NATIVE": "1"}


def _native(build, x, y, init, steps, fused=True, graph=True, clip=None, **env):
    w, h, eng, _ = _train(build, x, y, init, 32, steps, native=True, fused=fused, graph=graph,
                          optimizer=lambda: O.SGD(learning_rate=LR, **(clip or {})), extra_env={**STRICT, **env})
    assert eng == "native_graph", eng
    return w, h


def _calibrate(init, w_plain):
    """Per-variable gradients (fp64) and their norms from an unclipped SGD step."""
    grads = [-(b.astype(np.float64) - a) / LR for a, b in zip(init, w_plain)]
    return grads, [float(np.sqrt((g * g).sum())) for g in grads]


@pytest.fixture(scope="module")
def mnist_case():
    tf.set_seed(7)
    tf.keras.backend.clear_session()
    init = _mnist().get_weights()
    x, y = _data(96, (28, 28, 1), 10)
    # the unclipped native step (kept off the fused engine) calibrates every c below
    w_plain, h_plain = _native(_mnist, x, y, init, 1, fused=False)
    grads, norms = _calibrate(init, w_plain)
    allg = np.abs(np.concatenate([g.ravel() for g in grads]))
    c = {"clipvalue": float(np.median(allg[allg > 0])), "clipnorm": float(np.median(norms)),
         "global_clipnorm": 0.5 * math.sqrt(sum(v * v for v in norms))}
    return init, x, y, w_plain, h_plain, grads, norms, c


@pytest.mark.parametrize("mode", MODES)
def test_native_step_matches_closed_form(mnist_case, mode):
    init, x, y, w_plain, h_plain, grads, norms, cs = mnist_case
    c = cs[mode]
    # a clipped model under DAMD_FUSED=1 must land on native_graph (the fused engine rejects it)
    wc, hc = _native(_mnist, x, y, init, 1, clip={mode: c})
    assert hc == h_plain  # loss and metrics are the unclipped step's
    if mode == "clipnorm":
        clipped = [nv > c for nv in norms]
        assert any(clipped) and not all(clipped), norms
    for i, (a, b, got, g, nv) in enumerate(zip(init, w_plain, wc, grads, norms)):
        if mode == "global_clipnorm":
            want = 0.5 * (b.astype(np.float64) - a)
        elif mode == "clipnorm":
            want = (c / max(nv, c)) * (b.astype(np.float64) - a)
            if nv < c * (1 - 1e-5):
                np.testing.assert_array_equal(got, b)  # scale exactly 1: the plain step's bits
        else:
            want = -LR * np.clip(g, -c, c)
            assert (np.abs(g) > c).any(), i
        np.testing.assert_allclose(got.astype(np.float64) - a, want, atol=1e-6, rtol=0)
    # c far above the norm: bit-identical to the run without the argument
    wf, hf = _native(_mnist, x, y, init, 1, clip={mode: 1e6})
    for a, b in zip(wf, w_plain):
        np.testing.assert_array_equal(a, b)
    assert hf == h_plain


@pytest.mark.parametrize("mode", MODES)
def test_three_steps_track_the_generic_engine(mnist_case, mode):
    init, x, y, *_, cs = mnist_case
    w3, h3 = _native(_mnist, x, y, init, 3, clip={mode: cs[mode]})
    wg, hg, eng, _ = _train(_mnist, x, y, init, 32, 3, native=False, device="cpu",
                            optimizer=lambda: O.SGD(learning_rate=LR, **{mode: cs[mode]}))
    assert eng == "generic"
    print(mode, "3 steps: native", h3["loss"], "generic", hg["loss"])
    np.testing.assert_allclose(h3["loss"], hg["loss"], rtol=1e-2)


@pytest.mark.parametrize("mode", MODES)
def test_replay_and_buckets_are_bitwise(mnist_case, mode):
    init, x, y, *_, cs = mnist_case
    clip = {mode: cs[mode]}
    base, hb = _native(_mnist, x[:64], y[:64], init, 4, clip=clip)
    eager, he = _native(_mnist, x[:64], y[:64], init, 4, graph=False, clip=clip)
    for a, b in zip(base, eager):
        np.testing.assert_array_equal(a, b)
    assert hb == he
    # DAMD_BUCKET_OPT=1 with small buckets.  clipvalue: the per-bucket opt_step launches ==
    # the single launch; the norm modes fall back to the single update behind grad_norm
    bucketed, hk = _native(_mnist, x[:64], y[:64], init, 4, clip=clip, DAMD_BUCKET_OPT="1", DAMD_BUCKET_MB="0.05")
    for a, b in zip(base, bucketed):
        np.testing.assert_array_equal(a, b)
    assert hk == hb


def test_batchnorm_variables_clipnorm():
    tf.set_seed(9)
    tf.keras.backend.clear_session()
    build = TR._bn_net(False)
    init = build().get_weights()  # conv kernel, gamma, beta, moving mean, moving variance, dense kernel, bias
    rng = np.random.default_rng(6)
    init[1] = (1.0 + rng.normal(0, 0.2, 8)).astype(np.float32)
    init[2] = rng.normal(0, 0.3, 8).astype(np.float32)
    x, y = _data(32, (8, 8, 8), 10, seed=3)
    wp, hp = _native(build, x, y, init, 1)
    train = (0, 1, 2, 5, 6)
    grads, norms = _calibrate([init[i] for i in train], [wp[i] for i in train])
    c = float(np.median(norms))
    wc, hc = _native(build, x, y, init, 1, clip={"clipnorm": c})
    assert hc == hp
    assert norms[1] > 0 and norms[2] > 0  # gamma and beta carry a gradient
    clipped = [nv > c for nv in norms]
    assert any(clipped) and not all(clipped), norms
    for i, nv in zip(train, norms):
        want = (c / max(nv, c)) * (wp[i].astype(np.float64) - init[i])
        np.testing.assert_allclose(wc[i].astype(np.float64) - init[i], want, atol=1e-6, rtol=0)
        if nv < c * (1 - 1e-5):
            np.testing.assert_array_equal(wc[i], wp[i])
    for i in (3, 4):  # the moving statistics do not see the clipping
        np.testing.assert_array_equal(wc[i], wp[i])
