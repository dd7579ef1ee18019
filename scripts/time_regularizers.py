#!/usr/bin/env python
"""What weight regularizers cost on the native path, on one build and one GPU.

1. The ResNet-18 native training step (synthetic 224x224x3, 1000 classes, SGD momentum) with
   ``weight_decay=1e-4`` (an L2 regularizer on every conv / dense kernel: one reg_penalty
   launch per step and opt_step with the segment table) against ``weight_decay=None``, two
   engines in one process timed in alternating pairs of ``--steps`` graph replays each.
2. The two kernels alone at ResNet-18's parameter count and segment layout: ``reg_penalty``,
   and ``opt_step`` (SGD momentum) with and without the table, each as a captured graph of
   ``--launches`` launches replayed between two device events, alternating over the rounds.

Reported: the median over the rounds and the run-to-run spread (min, max, standard
deviation), one JSON line per part.

    python scripts/time_regularizers.py
    python scripts/time_regularizers.py --kernels-only --rounds 30
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(t, unit):
    return {f"median_{unit}": round(statistics.median(t), 4), f"min_{unit}": round(min(t), 4),
            f"max_{unit}": round(max(t), 4), f"stdev_{unit}": round(statistics.pstdev(t), 4)}


def time_steps(batch, steps, rounds, warmup, weight_decay):
    import distributed_amd as tf

    os.environ["DAMD_STRICT_NATIVE"] = "1"
    rows = 4 * batch
    rng = np.random.default_rng(1234)
    x = (rng.integers(0, 256, size=(rows, 224, 224, 3), dtype=np.uint8) / np.float32(255.0)).astype(np.float32)
    y = rng.integers(0, 1000, size=rows).astype(np.int64)
    engines = {}
    for name, wd in (("plain", None), ("regularized", weight_decay)):
        tf.set_seed(0)
        model = tf.models.resnet18(weight_decay=wd)
        tf.models.compile_resnet(model, 0.1, 0.9)
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
        for k, (_, eng) in engines.items():  # alternating pairs
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run(steps)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / steps)
    out = {"part": "resnet18_step", "batch": batch, "steps_per_window": steps, "rounds": rounds,
           "weight_decay": weight_decay,
           "reg_segments": engines["regularized"][1].describe_plan()["reg_segments"],
           "params": int(engines["plain"][1].nparam)}
    for k, t in times.items():
        out[k] = _stats(t, "ms_per_step")
    diffs = [b - a for a, b in zip(times["plain"], times["regularized"])]
    out["paired_difference"] = _stats(diffs, "ms_per_step")
    return out


def _graph_of(fn, launches):
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()  # (eager once: loads the code object)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for _ in range(launches):
                fn()
    torch.cuda.synchronize()
    return g


def _time(g, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches  # us per launch


def time_kernels(launches, rounds, warmup):
    """reg_penalty and opt_step (table on / off) over ResNet-18's flat buffer and table."""
    import distributed_amd as tf
    from distributed_amd.engine.ctrl import C_CUR3, C_LR, WORDS, f2i
    from distributed_amd.engine.native_plan import _pad8, reg_rows
    from distributed_amd.native import require_C
    from distributed_amd.ops import hip as H

    C, dev = require_C(), torch.device("cuda:0")
    vs = tf.models.resnet18(weight_decay=1e-4).trainable_weights  # (its layout and table only)
    offs, off = [], 0
    for v in vs:
        offs.append(off)
        off = _pad8(off + int(np.prod(v.shape)))
    n = off
    table = H.reg_table(reg_rows(vs, offs), dev)
    gen = torch.Generator().manual_seed(0)
    P = (torch.randn(n, generator=gen) * 0.05).to(dev)
    G = (torch.randn(n, generator=gen) * 0.01).to(dev)
    V = torch.zeros(n, device=dev)
    Pb = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    dummy = torch.zeros(8, device=dev)
    ctrl = torch.zeros(WORDS, dtype=torch.int32, device=dev)
    ctrl[C_LR], ctrl[C_CUR3] = f2i(1e-4), 1
    tail = torch.zeros(8, device=dev)
    scratch = H.reg_scratch(n, dev)

    def opt(reg):
        kw = dict(reg=table.data_ptr(), nreg=table.shape[0], lo=0) if reg else {}
        C.opt_step(P.data_ptr(), G.data_ptr(), V.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), Pb.data_ptr(), n,
                   ctrl.data_ptr(), tail.data_ptr(), 0, 0.0, 0.0, 0.0, 0.0, 0.9, 0,
                   torch.cuda.current_stream().cuda_stream, book=0, **kw)

    runs = {"reg_penalty": lambda: H.reg_penalty(P, table, scratch, tail=tail),
            "opt_step": lambda: opt(False), "opt_step_reg": lambda: opt(True)}
    graphs = {k: _graph_of(fn, launches) for k, fn in runs.items()}
    for _ in range(warmup):
        for g in graphs.values():
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():  # alternating
            times[k].append(_time(g, launches))
    out = {"part": "kernels", "params": n, "reg_segments": int(table.shape[0]), "launches": launches, "rounds": rounds,
           "reg_penalty_bytes_read": 4 * n}  # the whole flat buffer: the loads go out ahead of the row search
    for k, t in times.items():
        out[k] = _stats(t, "us")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20, help="graph replays per timed window")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--weight-decay", type=float, default=1e-4)
    ap.add_argument("--launches", type=int, default=200, help="kernel launches per captured graph")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_regularizers.py needs a HIP device")
    if not a.step_only:
        print(json.dumps(time_kernels(a.launches, a.rounds, a.warmup)), flush=True)
    if not a.kernels_only:
        print(json.dumps(time_steps(a.batch, a.steps, a.rounds, a.warmup, a.weight_decay)), flush=True)


if __name__ == "__main__":
    main()
