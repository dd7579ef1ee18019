"""SHA-256 digests of the fused MNIST step's results (csrc/kernels/convnet_step2.hip), for
tests/test_convnet_step_digests_gpu.py: a change to the step kernels that must keep every
bit is checked against digests recorded with the build of the commit BEFORE that change.

Scenario: B = 64 on 256 synthetic rows (fixed seed), eager launches, uint8 or fp32 rows, plain
SGD or momentum 0.9 + nesterov, the specialised (DAMD_SPECIALISED=1) or the generic kernels.
After steps 1 and 3: the pooled tile, the argmax codes, every weight and the epoch's metric
sums (loss, correct, count as the ctrl block holds them after the flush).

    python tests/helpers/step_digests.py --write   # records tests/golden/convnet_step_digests.json

Record only with a build of the parent commit, never with the code under test."""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden", "convnet_step_digests.json")
B, ROWS, SEED = 64, 256, 1234
CONFIGS = [(u8, opt) for u8 in (True, False) for opt in ("sgd", "nesterov")]


def config_id(u8: bool, opt: str) -> str:
    return f"{'u8' if u8 else 'fp32'}-{opt}"


def _sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _data(u8: bool):
    rng = np.random.default_rng(SEED)
    if u8:  # exactly k / 255: kept as uint8 rows on the device
        x = rng.integers(0, 256, (ROWS, 28, 28, 1)).astype(np.uint8) / 255.0
    else:
        x = rng.random((ROWS, 28, 28, 1), dtype=np.float32)
    return x, rng.integers(0, 10, ROWS).astype(np.int64)


def _snapshot(eng, model) -> dict:
    import torch

    from distributed_amd.engine.ctrl import C_AC, C_AL, C_AN  # epoch loss sum, correct, count (fp32 bits)

    eng.sync()  # (applies the pending update; the forward's outputs stay as step k left them)
    d = {"pooled": _sha(eng.pooled.view(torch.int16).cpu().numpy()), "code": _sha(eng.code.cpu().numpy())}
    for i, w in enumerate(model.get_weights()):
        d[f"w{i}"] = _sha(w)
    c = eng.ctrl.cpu().numpy()
    d["metrics"] = _sha(c[[C_AL, C_AC, C_AN]])
    return d


def run_arm(setenv, u8: bool, opt: str, specialised: bool) -> dict:
    """{"step1": {name: sha256}, "step3": {...}} of one arm; setenv(name, value) sets the
    engine's environment switches (pytest's monkeypatch.setenv, or os.environ.__setitem__)."""
    import distributed_amd as tf

    setenv("DAMD_X_U8", "1" if u8 else "0")
    setenv("DAMD_GRAPH", "0")
    setenv("DAMD_SPECIALISED", "1" if specialised else "0")
    tf.set_seed(SEED)
    m = tf.models.mnist_cnn()
    mom = 0.9 if opt == "nesterov" else 0.0
    m.compile(loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True),
              optimizer=tf.keras.optimizers.SGD(learning_rate=0.05, momentum=mom, nesterov=opt == "nesterov"),
              metrics=["accuracy"])
    x, y = _data(u8)
    eng = m._get_engine(B, B)
    assert eng.name == "fused_convnet", eng.name
    assert eng.step_kernels == ("specialised" if specialised else "generic"), eng.step_kernels
    eng.bind(x, y)
    assert eng.feed.x_u8 == u8
    eng.start_epoch(0, shuffle=False)
    eng.run(1)
    out = {"step1": _snapshot(eng, m)}
    eng.run(2)
    out["step3"] = _snapshot(eng, m)
    eng.finish()
    return out


def compute(setenv) -> dict:
    """config id -> {"specialised": arm, "generic": arm}"""
    return {config_id(u8, opt): {"specialised": run_arm(setenv, u8, opt, True),
                                 "generic": run_arm(setenv, u8, opt, False)} for u8, opt in CONFIGS}


def load_golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


def main(argv) -> int:
    sys.path.insert(0, ROOT)
    got = compute(os.environ.__setitem__)
    for cid, arms in got.items():
        if arms["specialised"] != arms["generic"]:
            print(f"{cid}: the two instantiations disagree; nothing recorded", file=sys.stderr)
            return 1
    digests = {cid: arms["specialised"] for cid, arms in got.items()}
    if "--write" in argv:
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        with open(GOLDEN, "w") as f:
            json.dump(digests, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", GOLDEN)
        return 0
    want = load_golden()
    bad = [(cid, st, k) for cid in want for st in want[cid] for k in want[cid][st]
           if digests.get(cid, {}).get(st, {}).get(k) != want[cid][st][k]]
    print("differences:", bad if bad else "none")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
