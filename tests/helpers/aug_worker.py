"""A worker process of tests/test_augmentation.py: a small model behind ZeroPadding2D /
RandomCrop / RandomFlip trained for two steps under the launcher's TF_CONFIG on CPU/gloo.
Every rank builds the same initial weights and data; rank r writes its weights to
$DAMD_TEST_OUT/rank<r>.npz and the History to rank<r>.json."""
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
    w0 = [rng.normal(0, 0.3, (36, 8)).astype(np.float32), rng.normal(0, 0.2, 8).astype(np.float32),
          rng.normal(0, 0.3, (8, 3)).astype(np.float32), np.zeros(3, np.float32)]
    x = rng.random((16, 6, 6, 1)).astype(np.float32)
    y = rng.integers(0, 3, 16)
    with strategy.scope():
        m = K.Sequential([K.layers.ZeroPadding2D(1, input_shape=(6, 6, 1)), K.layers.RandomCrop(6, 6, seed=5),
                          K.layers.RandomFlip(), K.layers.Flatten(), K.layers.Dense(8, activation="relu"),
                          K.layers.Dense(3)])
        m.compile(optimizer=K.optimizers.SGD(0.1), loss=K.losses.SparseCategoricalCrossentropy(from_logits=True))
    m.set_weights(w0)
    h = m.fit(x, y, batch_size=per * world, epochs=1, steps_per_epoch=2, shuffle=False, verbose=0)
    np.savez(os.path.join(out, f"rank{rank}.npz"), **{str(i): w for i, w in enumerate(m.get_weights())})
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump({"world": world, "rank": rank, "loss": h.history["loss"],
                   "iterations": int(m.optimizer.iterations), "engine": m._engine.name}, f)
    from distributed_amd.parallel import runtime

    runtime.shutdown()


if __name__ == "__main__":
    main()
