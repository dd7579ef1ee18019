#!/usr/bin/env python
"""What the native depthwise / separable convolutions (DAMD_NATIVE_DEPTHWISE=1) cost next to
the PyTorch-ops fallback they replace, on one build and one GPU.

1. Each of ``dwconv_fwd`` / ``dwconv_dgrad`` / ``dwconv_wgrad`` alone at batch 64, 3 x 3 'same':
   112 x 112 x 64 stride 1, 56 x 56 x 128 stride 2, 14 x 14 x 512 stride 1 -- a captured graph of
   ``--launches`` launches replayed between two device events.  Reported with the bytes the
   algorithm must move (each activation operand read or written once; the taps are
   negligible), that over the time, and whether those tensors fit the 256 MiB L3 (then the
   replays run out of it, not HBM).  Alongside (part ``torch``): ``ops/reference.py
   depthwise_conv2d`` -- torch's grouped ``F.conv2d``, what the fallback runs -- forward, and
   forward + autograd backward (both gradients in one call), on the same values, as
   ``--launches`` eager calls between two events.  ``--torch-dtype fp32`` (the default) is what
   GenericEngine runs; ``bf16`` asks the vendor library for the same storage format as the
   native kernels (a library error is reported in the output, not raised).
2. The training step of a small separable CNN (32 x 32 x 3, batch 64, SGD momentum):
   Conv2D(32, 3, same, relu) -> 3 x [SeparableConv2D(64 / 128 / 128, 3, same, no bias) -> BN ->
   ReLU], the second with stride 2 -> GAP -> Dense(10), with the switch on (native_graph) and off
   (the fallback, GenericEngine), in alternating rounds of ``--steps`` steps in one process.

Reported: the median over the rounds and the run-to-run spread (min, max, standard
deviation), one JSON line per part.

    python scripts/time_depthwise.py
    python scripts/time_depthwise.py --kernels-only --rounds 30
    python scripts/time_depthwise.py --torch-only --torch-dtype bf16
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

L3_BYTES = 256 << 20
SHAPES = {"112x112x64_s1": (112, 64, 1), "56x56x128_s2": (56, 128, 2), "14x14x512_s1": (14, 512, 1)}


def _eager_us(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def _operands(batch, size, c, s, dev):
    from distributed_amd.ops import hip as H

    geo = H.pool_geo((batch, size, size, c), (3, 3), (s, s), "same")
    gen = torch.Generator(device=dev).manual_seed(size * 1000 + c)
    x = torch.randn(batch, size, size, c, device=dev, generator=gen).to(torch.bfloat16)
    w = torch.randn(3, 3, c, 1, device=dev, generator=gen).to(torch.bfloat16)
    dy = torch.randn(batch, geo[10], geo[11], c, device=dev, generator=gen).to(torch.bfloat16)
    return geo, x, w, dy


def time_kernels(batch, launches, rounds, warmup):
    from distributed_amd.ops import hip as H

    dev = torch.device("cuda:0")
    graphs, nbytes = {}, {}
    # every tensor a captured graph touches stays referenced for as long as the graph: a capture
    # empties the allocator's cache, which hands unreferenced blocks back to the driver
    keep = []
    for name, (size, c, s) in SHAPES.items():
        geo, x, w, dy = _operands(batch, size, c, s, dev)
        y, dx = torch.zeros_like(dy), torch.zeros_like(x)
        dw = torch.zeros(3, 3, c, 1, device=dev)
        ws = torch.zeros(H.dwconv_wgrad_workspace_elems(geo), device=dev)
        keep += [x, w, dy, y, dx, dw, ws]
        graphs[f"{name}/fwd"] = _graph_of(lambda x=x, w=w, geo=geo, y=y: H.dwconv_fwd(x, w, None, False, geo, y),
                                          launches)
        graphs[f"{name}/dgrad"] = _graph_of(lambda dy=dy, w=w, geo=geo, dx=dx: H.dwconv_dgrad(dy, w, geo, dx),
                                            launches)
        graphs[f"{name}/wgrad"] = _graph_of(
            lambda x=x, dy=dy, geo=geo, dw=dw, ws=ws: H.dwconv_wgrad(x, dy, geo, dw, workspace=ws), launches)
        for k in ("fwd", "dgrad", "wgrad"):
            nbytes[f"{name}/{k}"] = (x.numel() + dy.numel()) * 2
    for _ in range(warmup):
        for g in graphs.values():
            g.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():  # alternating
            times[k].append(_time(g, launches))
    torch.cuda.synchronize()
    del keep
    out = {"part": "kernels", "batch": batch, "launches": launches, "rounds": rounds}
    for k, t in times.items():
        out[k] = _stats(t, "us")
        med = out[k]["median_us"]
        out[k].update(bytes_moved=nbytes[k], tb_per_s=round(nbytes[k] / med / 1e6, 3),
                      fits_l3=bool(nbytes[k] < L3_BYTES))
    for name in SHAPES:
        out[f"{name}/dgrad_plus_wgrad_us"] = round(out[f"{name}/dgrad"]["median_us"]
                                                   + out[f"{name}/wgrad"]["median_us"], 4)
    return out


def time_torch(batch, launches, rounds, warmup, dtype):
    from distributed_amd.ops import reference as R

    dev = torch.device("cuda:0")
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[dtype]
    out = {"part": "torch", "dtype": dtype, "batch": batch, "launches": launches, "rounds": rounds}
    for name, (size, c, s) in SHAPES.items():
        geo, x, w, dy = _operands(batch, size, c, s, dev)
        x, w, dy = x.to(dt), w.to(dt), dy.to(dt)
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)

        def fwd():
            with torch.no_grad():
                R.depthwise_conv2d(x, w, None, (s, s), "same")

        def fwd_bwd():
            torch.autograd.grad(R.depthwise_conv2d(xr, wr, None, (s, s), "same"), (xr, wr), dy)

        try:
            for _ in range(warmup):
                fwd()
                fwd_bwd()
            torch.cuda.synchronize()
            tf_, tb_ = [], []
            for _ in range(rounds):
                tf_.append(_eager_us(fwd, launches))
                tb_.append(_eager_us(fwd_bwd, launches))
        except RuntimeError as e:  # the vendor library has no kernel for this dtype / shape
            out[name] = {"not_measured": str(e).splitlines()[0][:200]}
            break  # (nothing more is started on the device after a library error)
        out[f"{name}/fwd"] = _stats(tf_, "us")
        out[f"{name}/fwd_bwd"] = _stats(tb_, "us")
        out[f"{name}/bwd_by_difference_us"] = round(out[f"{name}/fwd_bwd"]["median_us"]
                                                    - out[f"{name}/fwd"]["median_us"], 4)
    return out


def separable_cnn():
    import distributed_amd as tf

    L = tf.keras.layers
    layers = [L.Conv2D(32, 3, padding="same", activation="relu", input_shape=(32, 32, 3))]
    for filters, stride in ((64, 1), (128, 2), (128, 1)):
        layers += [L.SeparableConv2D(filters, 3, strides=stride, padding="same", use_bias=False),
                   L.BatchNormalization(), L.ReLU()]
    return tf.keras.Sequential(layers + [L.GlobalAveragePooling2D(), L.Dense(10)])


def time_steps(batch, steps, rounds, warmup):
    import distributed_amd as tf

    K = tf.keras
    rows = steps * batch
    rng = np.random.default_rng(1234)
    x = (rng.integers(0, 256, size=(rows, 32, 32, 3), dtype=np.uint8) / np.float32(255.0)).astype(np.float32)
    y = rng.integers(0, 10, size=rows).astype(np.int64)
    engines = {}
    for name, switch in (("native", "1"), ("fallback", "0")):
        os.environ["DAMD_NATIVE_DEPTHWISE"] = switch
        os.environ["DAMD_STRICT_NATIVE"] = switch  # the fallback only where it is asked for
        tf.set_seed(0)
        K.backend.clear_session()
        model = separable_cnn()
        model.compile(loss=K.losses.SparseCategoricalCrossentropy(from_logits=True),
                      optimizer=K.optimizers.SGD(learning_rate=0.05, momentum=0.9), metrics=["accuracy"])
        eng = model._get_engine(batch, batch)
        assert eng.name == ("native_graph" if name == "native" else "generic"), eng.name
        eng.bind(x, y)
        engines[name] = (model, eng)

    def window(name, eng):
        # (a fresh epoch of exactly `steps` batches: the fallback engine stops at the end of the data)
        eng.start_epoch(0, False)
        eng.prepare(steps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run(steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for _ in range(warmup):
        for k, (_, eng) in engines.items():
            window(k, eng)
    times = {k: [] for k in engines}
    for _ in range(rounds):
        for k, (_, eng) in engines.items():  # alternating
            times[k].append(window(k, eng))
    out = {"part": "separable_cnn_32x32_step", "batch": batch, "steps_per_window": steps, "rounds": rounds}
    for k, t in times.items():
        out[k] = _stats(t, "ms_per_step")
    out["paired_difference"] = _stats([a - b for a, b in zip(times["native"], times["fallback"])], "ms_per_step")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20, help="training steps per timed window")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=50, help="kernel launches per captured graph")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--torch-only", action="store_true")
    ap.add_argument("--torch-dtype", choices=("fp32", "bf16"), default="fp32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_depthwise.py needs a HIP device")
    only = a.kernels_only or a.step_only or a.torch_only
    if a.kernels_only or not only:
        print(json.dumps(time_kernels(a.batch, a.launches, a.rounds, a.warmup)), flush=True)
    if a.torch_only or not only:
        print(json.dumps(time_torch(a.batch, a.launches, a.rounds, a.warmup, a.torch_dtype)), flush=True)
    if a.step_only or not only:
        print(json.dumps(time_steps(a.batch, a.steps, a.rounds, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
