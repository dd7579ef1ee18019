"""DepthwiseConv2D / SeparableConv2D through the native engines (DAMD_NATIVE_DEPTHWISE=1):
engine choice, bitwise graph-replay / eager / run-to-run agreement, one SGD step against the
fp32 re-execution of the lowered plan with the plan's bf16 storage points
(tests/helpers/plan_walker.py), and native predict / evaluate against the generic CPU path.

Model A is test_depthwise_api._model(): Conv2D -> DepthwiseConv2D(relu, bias) ->
SeparableConv2D(stride 2, relu, bias) -> GAP -> Dense.  Model B puts BatchNormalization behind
the separable layer's pointwise half (the conv-epilogue statistics, BN -> ReLU fused) and a
linear depthwise layer with a bias between it and the head."""
import logging
import os
import sys

import numpy as np
import pytest

import distributed_amd as tf
from distributed_amd.engine.native_infer import NativeInference

from test_depthwise_api import _model
from test_native_graph_gpu import _data, _train
from test_native_infer_gpu import _Env

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import plan_walker as W  # noqa: E402

pytestmark = pytest.mark.gpu

L = tf.keras.layers
BATCH, SEED = 16, 20240521
ON = {"DAMD_NATIVE_DEPTHWISE": "1", "DAMD_STRICT_NATIVE": "1"}
OFF = {"DAMD_NATIVE_DEPTHWISE": "0", "DAMD_STRICT_NATIVE": "0"}


def _model_b():
    tf.keras.backend.clear_session()
    return tf.keras.Sequential([
        L.Conv2D(8, 3, padding="same", activation="relu", input_shape=(8, 8, 3)),
        L.SeparableConv2D(16, 3, strides=2, padding="same", use_bias=False), L.BatchNormalization(), L.ReLU(),
        L.DepthwiseConv2D(3, padding="same"), L.GlobalAveragePooling2D(), L.Dense(4)])


MODELS = {"A": _model, "B": _model_b}


def _init(build):
    tf.set_seed(SEED)
    return build().get_weights()


def _xy():
    return _data(4 * BATCH, (8, 8, 3), 4, seed=4)


class _Warnings(logging.Handler):
    def __init__(self):
        super().__init__(logging.WARNING)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


@pytest.mark.parametrize("name", ["A", "B"])
def test_engine_follows_the_switch(name):
    from distributed_amd.utils import logging as dlog

    build = MODELS[name]
    x, y = _xy()
    init = _init(build)
    _, h, eng = _train(build, x, y, init, BATCH, 1, native=True, extra_env=ON)
    assert eng == "native_graph" and np.isfinite(h["loss"][0])
    grab = _Warnings()
    dlog.get_logger().addHandler(grab)
    try:
        _, h, eng = _train(build, x, y, init, BATCH, 1, native=True, extra_env=OFF)
    finally:
        dlog.get_logger().removeHandler(grab)
    assert eng == "generic" and np.isfinite(h["loss"][0])
    layer = "DepthwiseConv2D" if name == "A" else "SeparableConv2D"  # the first one in layer order
    assert any("PyTorch eager fallback" in ln and f"layer {layer}" in ln for ln in grab.lines), grab.lines
    with pytest.raises(RuntimeError, match="DAMD_STRICT_NATIVE"):
        _train(build, x, y, init, BATCH, 1, native=True, extra_env=dict(OFF, DAMD_STRICT_NATIVE="1"))


@pytest.mark.parametrize("name", ["A", "B"])
def test_graph_replay_eager_and_repeated_runs_agree_bitwise(name):
    build = MODELS[name]
    x, y = _xy()
    init = _init(build)
    runs = [_train(build, x, y, init, BATCH, 3, native=True, momentum=0.9, graph=g, extra_env=ON)
            for g in (True, True, False)]
    assert all(r[2] == "native_graph" for r in runs)
    for other in runs[1:]:
        assert other[1]["loss"] == runs[0][1]["loss"]
        for a, b in zip(runs[0][0], other[0]):
            assert a.tobytes() == b.tobytes()
    assert any(np.abs(a - b).max() > 1e-5 for a, b in zip(runs[0][0], init))  # it trained


# scripts/sweep_dwconv_emulation.py: per variable of model A, the worst relative update error
# and the worst cosine between the emulated bf16 step and the plain fp32 step over 16 init seeds
EMULATION_VS_FP32 = {
    "conv2d/kernel:0": (1.4871e-01, 0.990343),
    "conv2d/bias:0": (1.8882e-01, 0.982085),
    "depthwise_conv2d/depthwise_kernel:0": (1.1819e-01, 0.994059),
    "depthwise_conv2d/bias:0": (2.0741e-01, 0.978270),
    "separable_conv2d/depthwise_kernel:0": (1.2611e-01, 0.992102),
    "separable_conv2d/pointwise_kernel:0": (8.0263e-02, 0.997368),
    "separable_conv2d/bias:0": (9.4876e-02, 0.996106),
    "dense/kernel:0": (1.4843e-02, 0.999935),
    "dense/bias:0": (8.5079e-03, 0.999986),
}


def test_model_a_step_matches_its_bf16_emulation():
    """One plain-SGD step (lr 0.1, batch 16) of model A on the native engine against the fp32
    torch re-execution of the engine's own plan that rounds where the plan stores bf16.  The two
    differ by summation order only (and the bf16 roundings a last-bit difference flips); the
    emulation differs from the plain fp32 step by every bf16 rounding.  That second distance,
    measured on the CPU with neither side running a native kernel --

        DAMD_DEVICE=cpu DAMD_NATIVE_DEPTHWISE=1 python scripts/sweep_dwconv_emulation.py --seeds 16

    gave, as the worst of 16 init seeds per variable, the relative update errors and cosines of
    EMULATION_VS_FP32 (relative error 0.0085 - 0.21, cosine 0.978 - 0.99999; relative loss
    difference <= 4.3e-5).  The native step must be at most twice as far from its emulation:
    relative error <= 2 rel, 1 - cosine <= 2 (1 - cos), per variable; the factor 2 covers the
    heavy tails of a 16-draw maximum.  (The two losses are printed, not compared.)"""
    from distributed_amd.parallel import runtime

    x, y = _data(BATCH, (8, 8, 3), 4, seed=4)
    lr = 0.1
    with _Env(DAMD_FUSED="0", DAMD_NATIVE_GRAPH="1", **ON):
        runtime.shutdown()
        try:
            tf.set_seed(SEED + 3)
            m = _model()
            m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=tf.keras.optimizers.SGD(learning_rate=lr), metrics=["accuracy"])
            e = m._get_engine(BATCH, BATCH)
            assert e.name == "native_graph"
            e.bind(x, y)
            e.start_epoch(0, False)
            w0 = {id(v): v.value.detach().cpu().clone() for v in m.trainable_weights}
            want, ref_loss = W.sgd_updates(e.plan, m, x, y, lr, quantize=True)
            e.run(1)
            e.sync()
            loss = e.metrics()["loss"]
            print(f"loss {loss:.6f} emulated {ref_loss:.6f}")
            bad = []
            for v in m.trainable_weights:
                rel, cos = W.update_distance(v.value.detach().cpu() - w0[id(v)], want[id(v)])
                rel_w, cos_w = EMULATION_VS_FP32[v.name]
                print(f"{v.name:40s} rel {rel:.3e} (bound {2 * rel_w:.3e})  1 - cos {1 - cos:.3e} "
                      f"(bound {2 * (1 - cos_w):.3e})")
                if not (rel <= 2 * rel_w and 1 - cos <= 2 * (1 - cos_w)):
                    bad.append(v.name)
            assert not bad, bad
            assert np.isfinite(loss)
        finally:
            runtime.shutdown()


def test_model_b_loss_falls_over_ten_steps():
    """BatchNormalization behind the pointwise half: ten steps on the same batch (one step per
    epoch, no shuffling), finite and falling."""
    from distributed_amd.parallel import runtime

    x, y = _data(BATCH, (8, 8, 3), 4, seed=4)
    init = _init(_model_b)
    with _Env(DAMD_FUSED="0", DAMD_NATIVE_GRAPH="1", **ON):
        runtime.shutdown()
        try:
            m = _model_b()
            m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=tf.keras.optimizers.SGD(learning_rate=0.05, momentum=0.9), metrics=["accuracy"])
            m.set_weights(init)
            h = m.fit(x, y, batch_size=BATCH, epochs=10, steps_per_epoch=1, shuffle=False, verbose=0)
            assert m._engine.name == "native_graph"
            loss = h.history["loss"]
            print("loss", [round(v, 4) for v in loss])
            assert len(loss) == 10 and np.isfinite(loss).all() and loss[-1] < loss[0]
            assert all(np.isfinite(w).all() for w in m.get_weights())
        finally:
            runtime.shutdown()


# scripts/sweep_dwconv_emulation.py: forward-only, |emulated bf16 logits - fp32 logits| / max |logit|,
# the worst of 16 init seeds
FORWARD_EMULATION = {"A": 1.254e-2, "B": 1.291e-2}


def _infer(build, weights, x, y, env):
    from distributed_amd.parallel import runtime

    with _Env(**env):
        runtime.shutdown()
        try:
            m = build()
            m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=tf.keras.optimizers.SGD(learning_rate=0.1), metrics=["accuracy"])
            m.set_weights(weights)
            logits = m.predict(x, batch_size=BATCH)
            ev = m.evaluate(x, y, batch_size=BATCH, verbose=0, return_dict=True)
            plans = list(getattr(m, "_infer_plans", {}).values())
            return np.asarray(logits), ev, plans
        finally:
            runtime.shutdown()


@pytest.mark.parametrize("name", ["A", "B"])
def test_native_predict_and_evaluate_match_the_generic_cpu_path(name):
    """Weights after three native training steps (so the BatchNorm moving statistics and every
    kernel have moved), then predict / evaluate on 40 rows -- a short last batch -- through
    native_infer against the same model on the generic CPU path (fp32).

    Logits within 2^-7 of max |logit|: one bf16 ulp (2^-8 relative) on each of two stored
    activations ahead of the fp32 logits.  That accounting is not a property of the storage
    format: the forward-only emulation of the inference plan against the same walk in fp32, on
    the CPU at the init weights (scripts/sweep_dwconv_emulation.py, worst of 16 seeds), is
    1.254e-2 of max |logit| for model A and 1.291e-2 for model B (FORWARD_EMULATION) -- these
    plans store six bf16 tensors ahead of the logits and read bf16 weight shadows, and the logits
    of a barely trained net are small sums of cancelling terms, so max |logit| is a small
    yardstick.  At this test's weights and rows the native logits are inside 2^-7 all the same
    (MI355X: 2.2e-3 of max |logit| for model A, 1.4e-3 for model B; the kernels are bitwise
    reproducible, so these do not move from run to run), and 2^-7 is what is asserted.  The
    loss follows from the logits (cross-entropy moves by at most twice the largest logit
    change); a row's prediction may only differ where the reference's top-two margin is inside
    twice the bound."""
    build = MODELS[name]
    x, y = _xy()
    w, _, eng = _train(build, x, y, _init(build), BATCH, 3, native=True, momentum=0.9, extra_env=ON)
    assert eng == "native_graph"
    x, y = x[:40], y[:40]
    nat, ev_n, plans = _infer(build, w, x, y, dict(ON, DAMD_NATIVE_INFER="1"))
    assert plans and all(isinstance(p, NativeInference) for p in plans)
    assert any(nd.kind == "DepthwiseConv2D" for p in plans for nd in p.plan.live)
    ref, ev_r, _ = _infer(build, w, x, y, dict(OFF, DAMD_DEVICE="cpu", DAMD_NATIVE_INFER="0"))
    assert nat.shape == ref.shape == (40, 4)
    bound = 2.0 ** -7 * np.abs(ref).max()
    err = np.abs(nat - ref).max()
    print(f"max |native - cpu| {err:.3e}, bound {bound:.3e} ({err / np.abs(ref).max():.3e} of max |logit|; the "
          f"emulation's own worst over init seeds: {FORWARD_EMULATION[name]:.3e})")
    assert err <= bound
    assert abs(ev_n["loss"] - ev_r["loss"]) <= 2 * bound
    top = np.sort(ref, axis=1)
    close = int(((top[:, -1] - top[:, -2]) < 2 * bound).sum())
    assert abs(ev_n["accuracy"] - ev_r["accuracy"]) <= close / 40 + 1e-9
