#!/usr/bin/env python
"""Device time of the two loss heads on the same shape in one process: softmax_xent (class
ids) and softmax_xent_dense (one-hot rows, label smoothing), each as the training step
launches it (bias-gradient fold on where colsum runs as one split).

Each timing is a captured graph of ``--launches`` back-to-back launches replayed between two
device events (an eager loop of a ~5 us kernel measures the launch rate, not the kernel),
after a warm-up; the two kernels alternate over ``--rounds`` rounds, so both see the same
machine state.  Reported per kernel: the median over the rounds and its run-to-run spread
(min, max, standard deviation), in microseconds per launch.

    python scripts/time_loss_head.py --shape 64,1000,1000 --shape 64,10,16
    python scripts/time_loss_head.py --sparse-only     # a tree without the dense kernel
    python scripts/time_loss_head.py --weighted        # both kernels with per-row weights

``--weighted`` times the W = true instantiations instead (keys ``<kernel>+w``): the same two
launches with a ``weights=`` array of B distinct values, in the same two-graph alternation.
Compare it with a run without the flag in the same session: what a graph measures depends on
which graphs it alternates with (all four in one process put 0.07 us on the unweighted sparse
kernel at 64 x 1000 and took 0.05 us off the weighted one), so the two arms are two runs.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def measure(H, B, K, ld, eps, launches, rounds, warmup, sparse_only, weighted=False):
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    z = torch.randn(B, ld, generator=gen).to(dev)
    ids = torch.randint(0, K, (B,), generator=gen)
    lab = ids.to(dev).to(torch.int32)
    y = torch.nn.functional.one_hot(ids, K).float().to(dev).contiguous()
    dl = torch.zeros(B, ld, dtype=torch.bfloat16, device=dev)
    tail = torch.zeros(3, device=dev)
    rows = H.xent_rows(B, dev)
    bg = torch.zeros(K, device=dev) if H.softmax_bias_fold_ok(B, K) else None
    # (the unweighted launches pass no weights argument: the script also runs on trees without one)
    kw, tag = {}, ""
    if weighted:
        kw, tag = {"weights": (0.25 + 0.05 * torch.arange(B, dtype=torch.float32)).to(dev)}, "+w"
    runs = {"softmax_xent" + tag: lambda: H.softmax_xent(z, lab, K, 1.0 / B, dl, tail, rows=rows, bias_grad=bg, **kw)}
    if not sparse_only:
        runs["softmax_xent_dense" + tag] = lambda: H.softmax_xent_dense(z, y, K, 1.0 / B, dl, tail, label_smoothing=eps,
                                                                        rows=rows, bias_grad=bg, **kw)
    graphs = {k: _graph_of(fn, launches) for k, fn in runs.items()}
    for _ in range(warmup):
        for g in graphs.values():
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():  # alternating
            times[k].append(_time(g, launches))
    out = {"shape": [B, K, ld], "label_smoothing": eps, "launches": launches, "rounds": rounds,
           "bias_fold": bg is not None}
    for k, t in times.items():
        out[k] = {"median_us": round(statistics.median(t), 3), "min_us": round(min(t), 3),
                  "max_us": round(max(t), 3), "stdev_us": round(statistics.pstdev(t), 3)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", action="append", help="B,K,ld (repeatable; default 64,1000,1000 and 64,10,16)")
    ap.add_argument("--label-smoothing", type=float, default=0.1)
    ap.add_argument("--launches", type=int, default=1000, help="launches per captured graph")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sparse-only", action="store_true")
    ap.add_argument("--weighted", action="store_true", help="time both kernels with per-row weights")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_loss_head.py needs a HIP device")
    from distributed_amd.ops import hip as H

    shapes = [tuple(int(v) for v in s.split(",")) for s in (a.shape or ["64,1000,1000", "64,10,16"])]
    for B, K, ld in shapes:
        print(json.dumps(measure(H, B, K, ld, a.label_smoothing, a.launches, a.rounds, a.warmup, a.sparse_only,
                                 a.weighted)),
              flush=True)


if __name__ == "__main__":
    main()
