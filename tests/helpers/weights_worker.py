"""A worker process of tests/test_sample_weights.py: a small dense model trained for two
shuffled epochs under the launcher's TF_CONFIG on CPU/gloo with per-sample weights (once as
sample_weight, once as sample_weight times class_weight) and once unweighted.  Every rank
builds the same initial weights and data; rank r writes its weights to
$DAMD_TEST_OUT/rank<r>.npz (keys "<run>/<i>") and the History to rank<r>.json."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
os.environ.setdefault("DAMD_DEVICE", "cpu")

import numpy as np  # noqa: E402

import distributed_amd as tf  # noqa: E402


def main():
    out = os.environ["DAMD_TEST_OUT"]
    per = int(os.environ.get("DAMD_TEST_PER_REPLICA", "4"))
    strategy = tf.distribute.experimental.MultiWorkerMirroredStrategy()
    world, rank = strategy.num_replicas_in_sync, strategy.rank
    K = tf.keras
    rng = np.random.default_rng(23)
    w0 = [rng.normal(0, 0.3, (16, 8)).astype(np.float32), rng.normal(0, 0.2, 8).astype(np.float32),
          rng.normal(0, 0.3, (8, 3)).astype(np.float32), np.zeros(3, np.float32)]
    x = rng.random((24, 4, 4, 1)).astype(np.float32)
    y = rng.integers(0, 3, 24)
    sw = rng.uniform(0.0, 3.0, 24).astype(np.float32)
    sw[[1, 7, 13]] = 0.0
    runs = {"none": {}, "sample": {"sample_weight": sw},
            "both": {"sample_weight": sw, "class_weight": {0: 1.0, 1: 2.5, 2: 0.5}}}
    weights, hist = {}, {}
    for name, kw in runs.items():
        tf.set_seed(5)  # the same epoch permutations in every run and at every world size
        with strategy.scope():
            m = K.Sequential([K.layers.Flatten(input_shape=(4, 4, 1)), K.layers.Dense(8), K.layers.Dense(3)])
            m.compile(optimizer=K.optimizers.SGD(0.1), metrics=["accuracy"],
                      loss=K.losses.SparseCategoricalCrossentropy(from_logits=True))
        m.set_weights(w0)
        h = m.fit(x, y, batch_size=per * world, epochs=2, shuffle=True, verbose=0, **kw)
        for i, w in enumerate(m.get_weights()):
            weights[f"{name}/{i}"] = w
        hist[name] = {"loss": h.history["loss"], "accuracy": h.history["accuracy"],
                      "iterations": int(m.optimizer.iterations), "engine": m._engine.name}
    np.savez(os.path.join(out, f"rank{rank}.npz"), **weights)
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump({"world": world, "rank": rank, "runs": hist}, f)
    from distributed_amd.parallel import runtime

    runtime.shutdown()


if __name__ == "__main__":
    main()
