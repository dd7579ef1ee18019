#!/usr/bin/env python
"""What gradient clipping costs on the native path, on one build and one GPU.

1. The ResNet-18 native training step (synthetic 224x224x3, 1000 classes, SGD momentum) with
   ``global_clipnorm``, with ``clipnorm`` (each: one grad_norm launch per step and opt_step
   with scales), with ``clipvalue`` (opt_step alone) and with neither; four engines in one
   process timed in alternating rounds of ``--steps`` graph replays each.
   ``--weight-decay 1e-4`` adds the L2 regularizer to all four (grad_norm then reads the
   masters of the regularized variables as well).
2. ``grad_norm`` alone over ResNet-18's flat buffer, per variable and global, without and
   with the regularizer coefficients, beside ``reg_penalty`` on the same buffer; each as a
   captured graph of ``--launches`` launches replayed between two device events,
   alternating over the rounds.

Reported: the median over the rounds and the run-to-run spread (min, max, standard
deviation), one JSON line per part.

    python scripts/time_clipping.py
    python scripts/time_clipping.py --kernels-only --rounds 30
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

# far above any norm of this workload: every scale is 1 and all four runs train alike (the
# cost of a launch does not depend on whether it clips)
CLIPS = (("plain", {}), ("global_clipnorm", {"global_clipnorm": 1e6}), ("clipnorm", {"clipnorm": 1e6}),
         ("clipvalue", {"clipvalue": 1e6}))


def time_steps(batch, steps, rounds, warmup, weight_decay):
    import distributed_amd as tf

    os.environ["DAMD_STRICT_NATIVE"] = "1"
    K = tf.keras
    rows = 4 * batch
    rng = np.random.default_rng(1234)
    x = (rng.integers(0, 256, size=(rows, 224, 224, 3), dtype=np.uint8) / np.float32(255.0)).astype(np.float32)
    y = rng.integers(0, 1000, size=rows).astype(np.int64)
    engines = {}
    for name, kw in CLIPS:
        tf.set_seed(0)
        model = tf.models.resnet18(weight_decay=weight_decay)
        model.compile(loss=K.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=K.optimizers.SGD(learning_rate=0.1, momentum=0.9, **kw), metrics=["accuracy"])
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
            times[k].append((time.perf_counter() - t0) * 1e3 / steps)
    plan = engines["clipnorm"][1].clip_plan
    out = {"part": "resnet18_step", "batch": batch, "steps_per_window": steps, "rounds": rounds,
           "weight_decay": weight_decay, "params": int(engines["plain"][1].nparam), "variables": plan.nvar,
           "chunks": plan.nchunk, "grad_norm_bytes_read": plan.bytes_read}
    for k, t in times.items():
        out[k] = _stats(t, "ms_per_step")
    for k in times:
        if k != "plain":
            out[f"paired_difference_{k}"] = _stats([b - a for a, b in zip(times["plain"], times[k])], "ms_per_step")
    return out


def time_kernels(launches, rounds, warmup):
    """grad_norm (per variable / global, without / with coefficients) and reg_penalty over
    ResNet-18's flat buffer."""
    import distributed_amd as tf
    from distributed_amd.engine.native_plan import _pad8, reg_rows
    from distributed_amd.ops import hip as H

    dev = torch.device("cuda:0")
    vs = tf.models.resnet18(weight_decay=1e-4).trainable_weights  # (its layout and table only)
    sizes = [int(np.prod(v.shape)) for v in vs]
    offs, off = [], 0
    for sz in sizes:
        offs.append(off)
        off = _pad8(off + sz)
    n = off
    rrows = reg_rows(vs, offs)
    co = {r[0]: (r[2], r[3]) for r in rrows}
    gen = torch.Generator().manual_seed(0)
    P, G = torch.zeros(n), torch.zeros(n)
    for o, sz in zip(offs, sizes):  # the padding between variables stays zero
        P[o:o + sz] = torch.randn(sz, generator=gen) * 0.05
        G[o:o + sz] = torch.randn(sz, generator=gen) * 0.01
    P, G = P.to(dev), G.to(dev)
    table, scratch = H.reg_table(rrows, dev), H.reg_scratch(n, dev)
    plans = {(pv, reg): H.clip_plan([(o, sz) + (co.get(o, (0.0, 0.0)) if reg else (0.0, 0.0))
                                     for o, sz in zip(offs, sizes)], n, dev, per_variable=pv)
             for pv in (True, False) for reg in (False, True)}
    runs = {"reg_penalty": lambda: H.reg_penalty(P, table, scratch)}
    for (pv, reg), plan in plans.items():
        name = ("grad_norm_per_variable" if pv else "grad_norm_global") + ("_reg" if reg else "")
        runs[name] = (lambda plan=plan, reg=reg: H.grad_norm(G, plan, 1.0, P=P if reg else None))
    graphs = {k: _graph_of(fn, launches) for k, fn in runs.items()}
    for _ in range(warmup):
        for g in graphs.values():
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():  # alternating
            times[k].append(_time(g, launches))
    any_plan = plans[(True, True)]
    out = {"part": "kernels", "params": n, "variables": any_plan.nvar, "chunks": any_plan.nchunk,
           "reg_segments": int(table.shape[0]), "launches": launches, "rounds": rounds,
           "reg_penalty_bytes_read": 4 * n, "grad_norm_bytes_read": plans[(True, False)].bytes_read,
           "grad_norm_reg_bytes_read": any_plan.bytes_read}
    for k, t in times.items():
        out[k] = _stats(t, "us")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20, help="graph replays per timed window")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--weight-decay", type=float, default=None)
    ap.add_argument("--launches", type=int, default=200, help="kernel launches per captured graph")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_clipping.py needs a HIP device")
    if not a.step_only:
        print(json.dumps(time_kernels(a.launches, a.rounds, a.warmup)), flush=True)
    if not a.kernels_only:
        print(json.dumps(time_steps(a.batch, a.steps, a.rounds, a.warmup, a.weight_decay)), flush=True)


if __name__ == "__main__":
    main()
