"""How far bf16 storage moves one SGD step of the depthwise / separable test model (CPU only):
the fp32 re-execution of the lowered plan with rounding at the plan's storage points
(tests/helpers/plan_walker.py) against the same walk without any rounding, over --seeds init
seeds.  Prints, per variable, the worst relative update error and the worst cosine -- the
yardstick of tests/test_dwconv_train_gpu.py, where the native step is held to twice these
distances from its emulation.  Neither side of this comparison runs a native kernel.

    DAMD_DEVICE=cpu DAMD_NATIVE_DEPTHWISE=1 python scripts/sweep_dwconv_emulation.py --seeds 16
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "helpers")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import distributed_amd as tf  # noqa: E402
from distributed_amd.engine.native_plan import lower  # noqa: E402

import plan_walker as W  # noqa: E402
from test_depthwise_api import _model  # noqa: E402
from test_dwconv_train_gpu import _model_b  # noqa: E402
from test_native_graph_gpu import _data  # noqa: E402

BATCH, LR, SEED0 = 16, 0.1, 20240521


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=16)
    a = ap.parse_args()
    x, y = _data(BATCH, (8, 8, 3), 4, seed=4)
    worst = {}
    for s in range(a.seeds):
        tf.set_seed(SEED0 + s)
        m = _model()
        plan = lower(m, BATCH)
        emu, le = W.sgd_updates(plan, m, x, y, LR, quantize=True)
        f32, lf = W.sgd_updates(plan, m, x, y, LR, quantize=False)
        for v in m.trainable_weights:
            rel, cos = W.update_distance(emu[id(v)], f32[id(v)])
            key = (m.trainable_weights.index(v), v.name)
            r0, c0, l0 = worst.get(key, (0.0, 1.0, 0.0))
            worst[key] = (max(r0, rel), min(c0, cos), max(l0, abs(le - lf) / abs(lf)))
    print(f"{a.seeds} seeds from {SEED0}: worst relative update error, worst cosine (emulated bf16 vs fp32)")
    for (i, nm), (rel, cos, dl) in sorted(worst.items()):
        print(f"  {i} {nm:40s} rel {rel:.4e}  cos {cos:.6f}")
    print(f"  worst relative loss difference {max(v[2] for v in worst.values()):.3e}")
    # forward only (the inference plan): emulated logits against fp32 logits, relative to max |logit|
    for name, build in (("A", _model), ("B", _model_b)):
        errs = []
        for s in range(a.seeds):
            tf.set_seed(SEED0 + s)
            m = build()
            plan = lower(m, BATCH, inference=True)
            leaves = {id(v): v.value.detach().float().cpu() for v in m.trainable_weights}
            with torch.no_grad():
                q = W.logits_of(plan, leaves, x, quantize=True, training=False)
                f = W.logits_of(plan, leaves, x, quantize=False, training=False)
            errs.append(float((q - f).abs().max() / f.abs().max()))
        print(f"model {name}: forward |emulated - fp32| / max |logit|: worst {max(errs):.3e} (2^-7 = {2 ** -7:.3e})")


if __name__ == "__main__":
    main()
