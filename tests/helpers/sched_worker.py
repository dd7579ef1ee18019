"""A worker process of tests/test_lr_schedules.py: a small dense model trained for three
steps under the launcher's TF_CONFIG on CPU/gloo, once per learning-rate schedule and once
at the constant initial rate.  Every rank builds the same initial weights and data; rank r
writes its weights to $DAMD_TEST_OUT/rank<r>.npz (keys "<run>/<i>") and the History to
rank<r>.json."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
os.environ.setdefault("DAMD_DEVICE", "cpu")

import numpy as np  # noqa: E402

import distributed_amd as tf  # noqa: E402

S = tf.keras.optimizers.schedules
# every one leaves the initial rate within the three steps (the test asserts that they did)
RUNS = {"none": lambda: 0.1,
        "exponential": lambda: S.ExponentialDecay(0.1, 2, 0.5),
        "inverse_time": lambda: S.InverseTimeDecay(0.1, 1, 0.5, staircase=True),
        "polynomial": lambda: S.PolynomialDecay(0.1, 2, 0.01, power=2.0, cycle=True),
        "piecewise": lambda: S.PiecewiseConstantDecay([0, 1], [0.1, 0.05, 0.2]),
        "cosine": lambda: S.CosineDecay(0.02, 4, alpha=0.1, warmup_target=0.1, warmup_steps=2)}


def main():
    out = os.environ["DAMD_TEST_OUT"]
    per = int(os.environ.get("DAMD_TEST_PER_REPLICA", "4"))
    strategy = tf.distribute.experimental.MultiWorkerMirroredStrategy()
    world, rank = strategy.num_replicas_in_sync, strategy.rank
    K = tf.keras
    rng = np.random.default_rng(11)
    w0 = [rng.normal(0, 0.3, (16, 8)).astype(np.float32), rng.normal(0, 0.2, 8).astype(np.float32),
          rng.normal(0, 0.3, (8, 3)).astype(np.float32), np.zeros(3, np.float32)]
    x = rng.random((24, 4, 4, 1)).astype(np.float32)
    y = rng.integers(0, 3, 24)
    weights, hist = {}, {}
    for name, make in RUNS.items():
        with strategy.scope():
            m = K.Sequential([K.layers.Flatten(input_shape=(4, 4, 1)), K.layers.Dense(8), K.layers.Dense(3)])
            m.compile(optimizer=K.optimizers.SGD(make(), momentum=0.9),
                      loss=K.losses.SparseCategoricalCrossentropy(from_logits=True))
        m.set_weights(w0)
        h = m.fit(x, y, batch_size=per * world, epochs=1, steps_per_epoch=3, shuffle=False, verbose=0)
        for i, w in enumerate(m.get_weights()):
            weights[f"{name}/{i}"] = w
        hist[name] = {"loss": h.history["loss"], "iterations": int(m.optimizer.iterations),
                      "engine": m._engine.name}
    np.savez(os.path.join(out, f"rank{rank}.npz"), **weights)
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump({"world": world, "rank": rank, "runs": hist}, f)
    from distributed_amd.parallel import runtime

    runtime.shutdown()


if __name__ == "__main__":
    main()
