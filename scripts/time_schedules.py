#!/usr/bin/env python
"""What a learning-rate schedule costs on the native graph engine, on one build and one GPU.

The reference MNIST CNN's native-graph training step (``DAMD_FUSED=0``, synthetic 28x28x1, SGD
momentum, graph replay, world 1) with a float rate and with ``CosineDecay`` (warm-up
included) evaluated inside the optimizer kernel: two engines in one process timed in
alternating rounds of ``--steps`` graph replays each.  ``--float-only`` times two float-rate
engines instead (their difference is the pairing's own noise; it also runs on a tree
without schedules).

Reported: the median over the rounds and the run-to-run spread (min, max, standard
deviation), one JSON line.

    python scripts/time_schedules.py
    python scripts/time_schedules.py --float-only
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_regularizers import _stats  # noqa: E402


def time_steps(batch, steps, rounds, warmup, float_only):
    os.environ["DAMD_STRICT_NATIVE"] = "1"
    os.environ["DAMD_FUSED"] = "0"
    import distributed_amd as tf

    K = tf.keras
    rows = 16 * batch
    rng = np.random.default_rng(1234)
    x = (rng.integers(0, 256, size=(rows, 28, 28, 1), dtype=np.uint8) / np.float32(255.0)).astype(np.float32)
    y = rng.integers(0, 10, size=rows).astype(np.int64)
    rates = {"float": lambda: 0.01}
    if float_only:
        rates["float_b"] = lambda: 0.01
    else:
        rates["cosine"] = lambda: K.optimizers.schedules.CosineDecay(0.001, 1 << 20, alpha=0.1, warmup_target=0.01,
                                                                     warmup_steps=1000)
    engines = {}
    for name, rate in rates.items():
        tf.set_seed(0)
        model = tf.models.mnist_cnn()
        model.compile(loss=K.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=K.optimizers.SGD(learning_rate=rate(), momentum=0.9), metrics=["accuracy"])
        eng = model._get_engine(batch, batch)
        assert eng.name == "native_graph", eng.name
        eng.bind(x, y)
        eng.start_epoch(0, True, wrap_steps=len(x) // batch)
        eng.prepare(steps)
        engines[name] = (model, eng)
    for _ in range(warmup):
        for _, eng in engines.values():
            eng.run(steps)
    torch.cuda.synchronize()
    times = {k: [] for k in engines}
    for _ in range(rounds):
        for k, (_, eng) in engines.items():  # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run(steps)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e6 / steps)
    out = {"part": "mnist_native_step", "batch": batch, "steps_per_window": steps, "rounds": rounds,
           "params": int(engines["float"][1].nparam)}
    for k, t in times.items():
        out[k] = _stats(t, "us_per_step")
    other = [k for k in times if k != "float"][0]
    out[f"paired_difference_{other}"] = _stats([b - a for a, b in zip(times["float"], times[other])], "us_per_step")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200, help="graph replays per timed window")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--float-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_schedules.py needs a HIP device")
    print(json.dumps(time_steps(a.batch, a.steps, a.rounds, a.warmup, a.float_only)), flush=True)


if __name__ == "__main__":
    main()
