"""A worker process of tests/test_regularizers.py: a small regularized dense model trained
for two steps under the launcher's TF_CONFIG on CPU/gloo.  Every rank builds the same
initial weights and data; rank r writes its weights and History to
$DAMD_TEST_OUT/rank<r>.npz / .json."""
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
    K, R = tf.keras, tf.keras.regularizers
    rng = np.random.default_rng(11)
    w0 = [rng.normal(0, 0.3, (16, 8)).astype(np.float32), rng.normal(0, 0.2, 8).astype(np.float32),
          rng.normal(0, 0.3, (8, 3)).astype(np.float32), np.zeros(3, np.float32)]
    w0[0][1, 1] = 0.0
    x = rng.random((16, 4, 4, 1)).astype(np.float32)
    y = rng.integers(0, 3, 16)

    def build(reg):
        kw = dict(kernel_regularizer=R.l1_l2(0.02, 0.05), bias_regularizer=R.l1(0.1)) if reg else {}
        with strategy.scope():
            m = K.Sequential([K.layers.Flatten(input_shape=(4, 4, 1)), K.layers.Dense(8, **kw), K.layers.Dense(3)])
            m.compile(optimizer=K.optimizers.SGD(0.1), loss=K.losses.SparseCategoricalCrossentropy(from_logits=True))
        m.set_weights(w0)
        return m

    model = build(True)
    penalty0 = float(sum(float(t) for t in model.losses))
    first = model.fit(x[:per * world], y[:per * world], batch_size=per * world, epochs=1, shuffle=False, verbose=0)
    plain = build(False)
    first_plain = plain.fit(x[:per * world], y[:per * world], batch_size=per * world, epochs=1, shuffle=False,
                            verbose=0)
    model = build(True)
    h = model.fit(x, y, batch_size=per * world, epochs=1, steps_per_epoch=2, shuffle=False, verbose=0)
    np.savez(os.path.join(out, f"rank{rank}.npz"), *model.get_weights())
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump({"history": h.history, "world": world, "rank": rank, "penalty0": penalty0,
                   "first_step_loss": first.history["loss"][0], "first_step_data_loss": first_plain.history["loss"][0],
                   "iterations": int(model.optimizer.iterations)}, f)
    from distributed_amd.parallel import runtime

    runtime.shutdown()


if __name__ == "__main__":
    main()
