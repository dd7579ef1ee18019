#!/usr/bin/env python
"""What on-device input augmentation costs on the native path, on one build and one GPU.

1. The native training step of ``models.resnet18(input_shape=(32, 32, 3))`` (10 classes, SGD
   momentum, batch 64) with and without the input prefix ``ZeroPadding2D(4) -> RandomCrop(32,
   32) -> RandomFlip("horizontal")``: two engines in one process timed in alternating rounds
   of ``--steps`` graph replays each.
2. The ``augment`` launch alone at that shape (64 x 32 x 32, 4-channel pixels, the pad / crop
   / flip table) and at an ImageNet-size shape (64 x 256 x 256 -> crop 224 -> flip), each as
   a captured graph of ``--launches`` launches replayed between two device events.

Reported: the median over the rounds and the run-to-run spread (min, max, standard
deviation), one JSON line per part.

    python scripts/time_augmentation.py
    python scripts/time_augmentation.py --kernels-only --rounds 30
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

from time_regularizers import _graph_of, _stats, _time  # noqa: E402


def time_steps(batch, steps, rounds, warmup):
    import distributed_amd as tf

    os.environ["DAMD_STRICT_NATIVE"] = "1"
    K, L = tf.keras, tf.keras.layers
    rows = 16 * batch
    rng = np.random.default_rng(1234)
    x = (rng.integers(0, 256, size=(rows, 32, 32, 3), dtype=np.uint8) / np.float32(255.0)).astype(np.float32)
    y = rng.integers(0, 10, size=rows).astype(np.int64)
    engines = {}
    for name in ("plain", "augmented"):
        tf.set_seed(0)
        aug = [L.ZeroPadding2D(4), L.RandomCrop(32, 32), L.RandomFlip("horizontal")] if name == "augmented" else None
        model = tf.models.resnet18(10, input_shape=(32, 32, 3), augmentation=aug)
        model.compile(loss=K.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=K.optimizers.SGD(learning_rate=0.1, momentum=0.9), metrics=["accuracy"])
        eng = model._get_engine(batch, batch)
        assert eng.name == "native_graph", eng.name
        assert (eng.nodes[0].kind == "Augment") == (name == "augmented") and eng.cin_pad == 4
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
            times[k].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {"part": "resnet18_32x32_step", "batch": batch, "steps_per_window": steps, "rounds": rounds}
    for k, t in times.items():
        out[k] = _stats(t, "ms_per_step")
    out["paired_difference"] = _stats([b - a for a, b in zip(times["plain"], times["augmented"])], "ms_per_step")
    return out


def time_kernels(batch, launches, rounds, warmup):
    from distributed_amd.engine.ctrl import C_CUR3, WORDS
    from distributed_amd.ops import hip as H

    dev = torch.device("cuda:0")
    cases = {
        "augment_cifar_pad_crop_flip": (32, 4, [(H.AUG_PAD, 4, 4, 4, 4, 0), (H.AUG_CROP, 32, 32, 0, 0, 11),
                                                (H.AUG_FLIP, 1, 0, 0, 0, 12)], 32),
        "augment_imagenet_crop_flip": (256, 4, [(H.AUG_CROP, 224, 224, 0, 0, 11), (H.AUG_FLIP, 1, 0, 0, 0, 12)], 224),
    }
    ctrl = torch.zeros(WORDS, dtype=torch.int32)
    ctrl[C_CUR3] = 1
    ctrl = ctrl.to(dev)
    labels = torch.zeros(batch, dtype=torch.int32, device=dev)
    graphs, nbytes = {}, {}
    for name, (size, cp, stages, out) in cases.items():
        x = torch.randn(batch, size, size, cp, device=dev).to(torch.bfloat16)
        y = torch.zeros(batch, out, out, cp, dtype=torch.bfloat16, device=dev)
        tab = H.aug_table(stages)
        graphs[name] = _graph_of(lambda x=x, y=y, tab=tab: H.augment(x, y, labels, ctrl, tab, True), launches)
        nbytes[name] = 2 * y.numel() * 2  # every output pixel written once and read at most once
    for _ in range(warmup):
        for g in graphs.values():
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():  # alternating
            times[k].append(_time(g, launches))
    out = {"part": "kernels", "batch": batch, "launches": launches, "rounds": rounds}
    for k, t in times.items():
        out[k] = dict(_stats(t, "us"), bytes_moved=nbytes[k])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50, help="graph replays per timed window")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=200, help="kernel launches per captured graph")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_augmentation.py needs a HIP device")
    if not a.step_only:
        print(json.dumps(time_kernels(a.batch, a.launches, a.rounds, a.warmup)), flush=True)
    if not a.kernels_only:
        print(json.dumps(time_steps(a.batch, a.steps, a.rounds, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
