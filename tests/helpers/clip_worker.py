"""A worker process of tests/test_grad_clipping.py: a small dense model (one kernel with an
L2 penalty) trained for two steps under the launcher's TF_CONFIG on CPU/gloo, once per
clipping mode and once unclipped.  Every rank builds the same initial weights and data;
rank r writes its weights to $DAMD_TEST_OUT/rank<r>.npz (keys "<mode>/<i>") and the
History to rank<r>.json."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
os.environ.setdefault("DAMD_DEVICE", "cpu")

import numpy as np  # noqa: E402

import distributed_amd as tf  # noqa: E402

# small enough to clip at every step of this model (the test asserts that they do)
MODES = {"none": {}, "clipvalue": {"clipvalue": 0.01}, "clipnorm": {"clipnorm": 0.05},
         "global_clipnorm": {"global_clipnorm": 0.1}}


def main():
    out = os.environ["DAMD_TEST_OUT"]
    per = int(os.environ.get("DAMD_TEST_PER_REPLICA", "4"))
    strategy = tf.distribute.experimental.MultiWorkerMirroredStrategy()
    world, rank = strategy.num_replicas_in_sync, strategy.rank
    K, R = tf.keras, tf.keras.regularizers
    rng = np.random.default_rng(11)
    w0 = [rng.normal(0, 0.3, (16, 8)).astype(np.float32), rng.normal(0, 0.2, 8).astype(np.float32),
          rng.normal(0, 0.3, (8, 3)).astype(np.float32), np.zeros(3, np.float32)]
    x = rng.random((16, 4, 4, 1)).astype(np.float32)
    y = rng.integers(0, 3, 16)
    weights, hist = {}, {}
    for mode, kw in MODES.items():
        with strategy.scope():
            m = K.Sequential([K.layers.Flatten(input_shape=(4, 4, 1)),
                              K.layers.Dense(8, kernel_regularizer=R.l2(0.05)), K.layers.Dense(3)])
            m.compile(optimizer=K.optimizers.SGD(0.1, **kw),
                      loss=K.losses.SparseCategoricalCrossentropy(from_logits=True))
        m.set_weights(w0)
        h = m.fit(x, y, batch_size=per * world, epochs=1, steps_per_epoch=2, shuffle=False, verbose=0)
        for i, w in enumerate(m.get_weights()):
            weights[f"{mode}/{i}"] = w
        hist[mode] = {"loss": h.history["loss"], "iterations": int(m.optimizer.iterations),
                      "engine": m._engine.name}
    np.savez(os.path.join(out, f"rank{rank}.npz"), **weights)
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump({"world": world, "rank": rank, "runs": hist}, f)
    from distributed_amd.parallel import runtime

    runtime.shutdown()


if __name__ == "__main__":
    main()
