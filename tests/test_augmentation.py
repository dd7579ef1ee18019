"""Input augmentation on CPU: the RandomFlip / RandomCrop layers, the (seed, t, g) draws of the
host oracle (ops/hip.py augment_reference), the planner's input prefix, and the generic
engine (resume, world 2 == world 1)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from distributed_amd import keras, launch, r_api
from distributed_amd.engine.native_graph import NativeGraphEngine
from distributed_amd.engine.native_infer import NativeInference
from distributed_amd.keras import backend as K
from distributed_amd.models import resnet18
from distributed_amd.ops import hip as H

L = keras.layers
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "helpers", "aug_worker.py")


class _FakeGPUStrategy:
    device = torch.device("cuda")


def _images(b, h, w, c, seed=0):
    # every value distinct: a moved pixel cannot be mistaken for another
    return np.random.default_rng(seed).permutation(b * h * w * c).reshape(b, h, w, c).astype(np.float32) + 1.0


def _cifar_net(prefix=True, size=16, pad=2):
    ls = []
    kw = {"input_shape": (size, size, 3)}
    if prefix:
        ls += [L.ZeroPadding2D(pad, **kw), L.RandomCrop(size, size), L.RandomFlip("horizontal")]
        kw = {}
    ls += [L.Conv2D(8, 3, padding="same", activation="relu", **kw), L.MaxPooling2D(2), L.Flatten(), L.Dense(10)]
    m = keras.Sequential(ls)
    m.compile(optimizer=keras.optimizers.SGD(0.05, momentum=0.9),
              loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True), metrics=["accuracy"])
    return m


# --- 1. API --------------------------------------------------------------------------------------
def test_shapes_and_errors():
    assert L.RandomFlip().compute_output_shape((None, 8, 9, 3)) == (None, 8, 9, 3)
    assert L.RandomCrop(4, 6).compute_output_shape((None, 8, 9, 3)) == (None, 4, 6, 3)
    inp = L.Input((8, 9, 3))
    assert L.RandomCrop(4, 6)(L.RandomFlip("vertical")(L.ZeroPadding2D(1)(inp))).shape == (None, 4, 6, 3)
    for mode in ("horizontal", "vertical", "horizontal_and_vertical"):
        assert L.RandomFlip(mode).mode == mode
    assert L.RandomFlip().mode == "horizontal_and_vertical"
    for bad in ("both", "", None, "Horizontal"):
        with pytest.raises(ValueError):
            L.RandomFlip(bad)
    with pytest.raises(ValueError):  # built against a smaller input: no resize path
        L.RandomCrop(9, 4)(L.Input((8, 9, 3)))
    with pytest.raises(ValueError):
        L.RandomCrop(4, 10)(L.Input((8, 9, 3)))
    with pytest.raises(ValueError):
        keras.Sequential([L.RandomCrop(40, 40, input_shape=(32, 32, 3))])
    with pytest.raises(ValueError):
        L.RandomCrop(4, 4)(torch.zeros(2, 3, 5, 1), training=True)


def test_config_json_and_hdf5_round_trips(tmp_path):
    f, c = L.RandomFlip("vertical", seed=7, name="f"), L.RandomCrop(5, 6, seed=9, name="c")
    assert {k: f.get_config()[k] for k in ("mode", "seed", "name")} == {"mode": "vertical", "seed": 7, "name": "f"}
    assert {k: c.get_config()[k] for k in ("height", "width", "seed")} == {"height": 5, "width": 6, "seed": 9}
    f2, c2 = L.RandomFlip.from_config(f.get_config()), L.RandomCrop.from_config(c.get_config())
    assert (f2.mode, f2.seed, c2.height, c2.width, c2.seed) == ("vertical", 7, 5, 6, 9)
    assert L.LAYER_CLASSES["RandomFlip"] is L.RandomFlip and L.LAYER_CLASSES["RandomCrop"] is L.RandomCrop

    m = keras.Sequential([L.ZeroPadding2D(((1, 2), (3, 0)), input_shape=(8, 8, 3)), L.RandomCrop(6, 6, seed=3),
                          L.RandomFlip("horizontal"), L.Flatten(), L.Dense(4)])
    m.compile(optimizer="sgd", loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    path = str(tmp_path / "m.h5")
    m.save(path)
    x = _images(3, 8, 8, 3)
    for back in (keras.models.model_from_json(m.to_json()), keras.models.load_model(path)):
        assert [type(l).__name__ for l in back.layers] == [type(l).__name__ for l in m.layers]
        assert back.layers[0].padding == ((1, 2), (3, 0))
        assert (back.layers[1].height, back.layers[1].width, back.layers[1].seed) == (6, 6, 3)
        assert (back.layers[2].mode, back.layers[2].seed) == ("horizontal", None)
        assert back.output_shape == (None, 4)
        assert L.augment_seeds(back) == {id(b): L.augment_seeds(m)[id(a)] for a, b in zip(m.layers, back.layers)
                                         if id(a) in L.augment_seeds(m)}
    assert np.array_equal(keras.models.load_model(path).predict(x), m.predict(x))
    # functional models too
    inp = L.Input((8, 8, 3))
    fm = keras.Model(inp, L.Dense(2)(L.Flatten()(L.RandomFlip()(L.RandomCrop(4, 4)(inp)))))
    back = keras.models.model_from_json(fm.to_json())
    assert [type(l).__name__ for l in back.layers] == [type(l).__name__ for l in fm.layers]


def test_r_verbs():
    m = r_api.keras_model_sequential()
    m = r_api.layer_random_crop(m, height=4.0, width=6.0, seed=3.0)
    m = r_api.layer_random_flip(m, mode="horizontal")
    crop, flip = m.layers[-2:]
    assert type(crop) is L.RandomCrop and (crop.height, crop.width, crop.seed) == (4, 6, 3)
    assert type(flip) is L.RandomFlip and (flip.mode, flip.seed) == ("horizontal", None)
    assert type(r_api.layer_random_flip()) is L.RandomFlip
    with open(os.path.join(ROOT, "R", "NAMESPACE")) as f:
        exports = re.findall(r"^export\(\"?([^\")]+)\"?\)", f.read(), re.M)
    with open(os.path.join(ROOT, "R", "R", "keras_verbs.R")) as f:
        verbs = f.read()
    for v in ("layer_random_flip", "layer_random_crop"):
        assert v in exports and re.search(rf"^{v} <- function", verbs, re.M) and f".r()${v}(" in verbs


# --- 2. inference --------------------------------------------------------------------------------
def test_inference_is_identity_and_centre_crop():
    x = torch.from_numpy(_images(3, 7, 9, 2))
    assert torch.equal(L.RandomFlip()(x), x) and torch.equal(L.RandomFlip()(x, training=False), x)
    y = L.RandomCrop(4, 6)(x)
    assert torch.equal(y, x[:, 1:5, 1:7])  # (7 - 4) // 2 = 1, (9 - 6) // 2 = 1
    assert torch.equal(L.RandomCrop(7, 9)(x), x)
    stages = [(H.AUG_PAD, 1, 0, 0, 2, 0), (H.AUG_CROP, 4, 6, 0, 0, 11), (H.AUG_FLIP, 3, 0, 0, 0, 12)]
    ref = H.augment_reference(x.numpy(), stages, 5, 2, training=False)
    assert np.array_equal(ref, np.pad(x.numpy(), ((0, 0), (1, 0), (0, 2), (0, 0)))[:, 2:6, 2:8])


# --- 3. the draws (checked on the oracle) ----------------------------------------------------------
def _flips(mode, seed, ts, gs):
    """[len(ts), len(gs)] (left-right, up-down) decisions read off the oracle's output."""
    x = np.tile(np.arange(4, dtype=np.float32).reshape(1, 2, 2, 1), (len(gs), 1, 1, 1))  # [[0 1] [2 3]]
    lr, ud = [], []
    for t in ts:
        y = H.augment_reference(x, [(H.AUG_FLIP, mode, 0, 0, 0, seed)], t, gs[0], True)[:, :, :, 0]
        lr.append(y[:, 0, 0] % 2 == 1)
        ud.append(y[:, 0, 0] >= 2)
    return np.array(lr), np.array(ud)


def test_flip_rates_and_axis_independence():
    ts, gs = range(1, 65), range(64)
    for seed in (H.aug_seed(None, 0), H.aug_seed(1, 3)):
        lr, ud = _flips(3, seed, ts, gs)
        assert 0.45 <= lr.mean() <= 0.55 and 0.45 <= ud.mean() <= 0.55
        assert 0.40 <= (lr == ud).mean() <= 0.60
        lr1, ud1 = _flips(1, seed, ts, gs)
        assert np.array_equal(lr1, lr) and not ud1.any()  # "horizontal" never flips up-down
        lr2, ud2 = _flips(2, seed, ts, gs)
        assert np.array_equal(ud2, ud) and not lr2.any()


def test_crop_offsets_cover_the_range_and_stay_inside():
    x = _images(64, 7, 9, 1)
    seen = set()
    for t in range(1, 65):
        y = H.augment_reference(x, [(H.AUG_CROP, 4, 6, 0, 0, H.aug_seed(None, 1))], t, 0, True)
        assert y.shape == (64, 4, 6, 1)
        for b in range(64):
            oy, ox = np.argwhere(x[b, :, :, 0] == y[b, 0, 0, 0])[0]
            assert 0 <= oy <= 3 and 0 <= ox <= 3
            assert np.array_equal(y[b], x[b, oy:oy + 4, ox:ox + 6])
            seen.add((int(oy), int(ox)))
    assert seen == {(a, b) for a in range(4) for b in range(4)}


def test_draws_are_a_pure_function_of_seed_t_g():
    x = _images(8, 6, 6, 2)
    m = keras.Sequential([L.RandomFlip(input_shape=(6, 6, 2)), L.RandomFlip(), L.RandomCrop(4, 4), L.RandomCrop(3, 3)])
    seeds = L.augment_seeds(m)
    assert len(set(seeds.values())) == 4  # seed=None twice in one model: the position separates them
    a, b = ([(H.AUG_FLIP, 3, 0, 0, 0, seeds[id(l)])] for l in m.layers[:2])
    ya = np.stack([H.augment_reference(x, a, t, 0, True) for t in range(1, 17)])
    yb = np.stack([H.augment_reference(x, b, t, 0, True) for t in range(1, 17)])
    assert not np.array_equal(ya, yb)
    assert np.array_equal(ya, np.stack([H.augment_reference(x, a, t, 0, True) for t in range(1, 17)]))
    # slot g of a batch that starts at g0 is slot g of one that starts at 0; t matters
    full = H.augment_reference(np.concatenate([x, x]), a, 3, 0, True)
    assert np.array_equal(H.augment_reference(x, a, 3, 8, True), full[8:])
    assert not np.array_equal(H.augment_reference(x, a, 3, 0, True), H.augment_reference(x, a, 4, 0, True))
    assert H.aug_seed(None, 2) == H.aug_seed(H.AUG_DEFAULT_SEED, 2) != H.aug_seed(None, 3)
    assert 0 <= H.aug_seed(2**40 + 5, 7) < 2**32


# --- 4. the layers' torch path versus the oracle -----------------------------------------------------
@pytest.mark.parametrize("t,g0", [(1, 0), (2, 0), (1000003, 5)])
def test_layers_equal_the_oracle(t, g0):
    x = _images(6, 7, 9, 3)
    m = keras.Sequential([L.ZeroPadding2D(((1, 2), (3, 0)), input_shape=(7, 9, 3)), L.RandomCrop(4, 6, seed=2),
                          L.RandomFlip(), L.RandomFlip("horizontal", seed=4), L.RandomCrop(3, 3)])
    seeds = L.augment_seeds(m)
    stages, ho, wo = H.aug_stages(m.layers, seeds, 7, 9)
    assert (ho, wo) == (3, 3) and len(stages) == 5
    with K.AugmentContext(t, np.arange(g0, g0 + 6), seeds):
        y = torch.from_numpy(x)
        for i, l in enumerate(m.layers):
            xin = y
            y = l(xin, training=True)
            one, _, _ = H.aug_stages([l], seeds, xin.shape[1], xin.shape[2])
            assert np.array_equal(y.numpy(), H.augment_reference(xin.numpy(), one, t, g0, True)), type(l).__name__
            # independently: every sample is one of the layer's finitely many candidates
            for b in range(6):
                s = xin[b].numpy()
                if isinstance(l, L.RandomFlip):
                    cands = [s, s[:, ::-1]] + ([s[::-1], s[::-1, ::-1]] if l.mode != "horizontal" else [])
                elif isinstance(l, L.RandomCrop):
                    cands = [s[a:a + l.height, c:c + l.width] for a in range(s.shape[0] - l.height + 1)
                             for c in range(s.shape[1] - l.width + 1)]
                else:
                    cands = [np.pad(s, ((1, 2), (3, 0), (0, 0)))]
                assert any(np.array_equal(y[b].numpy(), c) for c in cands), (type(l).__name__, b)
        assert np.array_equal(y.numpy(), H.augment_reference(x, stages, t, g0, True))
    assert K.augment_context() is None


def test_bare_call_uses_t1_and_row_slots():
    x = _images(5, 6, 6, 1)
    f, c = L.RandomFlip(seed=3), L.RandomCrop(4, 4)
    assert np.array_equal(f(torch.from_numpy(x), training=True).numpy(),
                          H.augment_reference(x, [(H.AUG_FLIP, 3, 0, 0, 0, H.aug_seed(3, 0))], 1, 0, True))
    assert np.array_equal(c(torch.from_numpy(x), training=True).numpy(),
                          H.augment_reference(x, [(H.AUG_CROP, 4, 4, 0, 0, H.aug_seed(None, 0))], 1, 0, True))


def test_zero_band_inside_the_image():
    # crop -> pad -> crop: the pad band of the middle stage lies inside the final window
    x = _images(4, 6, 6, 1)
    stages = [(H.AUG_CROP, 3, 3, 0, 0, 1), (H.AUG_PAD, 2, 1, 1, 2, 0), (H.AUG_CROP, 5, 5, 0, 0, 2)]
    y = H.augment_reference(x, stages, 1, 0, True)
    assert y.shape == (4, 5, 5, 1)
    for b in range(4):
        nz = np.argwhere(y[b, :, :, 0] != 0)
        assert 0 < len(nz) <= 9 and (y[b] == 0).sum() >= 16
        assert set(y[b][y[b] != 0]) <= set(x[b].ravel())


# --- 5. the planner ---------------------------------------------------------------------------------
def test_prefix_plans_as_one_node():
    m = _cifar_net()
    st = _FakeGPUStrategy()
    assert NativeGraphEngine.eligible(m, st) == (True, "")
    assert NativeInference.eligible(m, "cuda") == (True, "")
    assert NativeInference.eligible(m, "cuda", evaluate=True) == (True, "")
    p = NativeGraphEngine.plan_only(m, 8)
    aug = [nd for nd in p.nodes if nd.kind == "Augment"]
    assert len(aug) == 1 and p.nodes[0] is aug[0] and not aug[0].attrs["dead"]
    assert [nd.kind for nd in p.nodes] == ["Augment", "Conv2D", "MaxPooling2D", "Flatten", "Dense"]
    assert aug[0].inputs == [p.x0] and p.x0.shape == (8, 16, 16, 8)
    assert aug[0].out.shape == (8, 16, 16, 8) and not aug[0].out.needs_grad
    assert p.nodes[1].inputs[0] is aug[0].out
    stages = aug[0].attrs["stages"]
    assert [s[0] for s in stages] == [H.AUG_PAD, H.AUG_CROP, H.AUG_FLIP]
    assert stages[0][1:5] == (2, 2, 2, 2) and stages[1][1:3] == (16, 16) and stages[2][1] == 1
    tab = aug[0].attrs["table"]
    assert tab.dtype == torch.int32 and not tab.is_cuda and tab.numel() == H.AUG_WORDS and int(tab[0]) == 3
    # a crop that changes the size
    m2 = keras.Sequential([L.RandomCrop(12, 12, input_shape=(16, 16, 3)), L.Conv2D(8, 3, padding="same"), L.Flatten(),
                           L.Dense(4)])
    p2 = NativeGraphEngine.plan_only(m2, 4)
    assert p2.x0.shape == (4, 16, 16, 8) and p2.nodes[0].out.shape == (4, 12, 12, 8)
    assert p2.nodes[1].out.shape == (4, 12, 12, 8)


def test_resnet18_behind_crop_and_flip_keeps_the_packed_stem():
    m = resnet18(10, input_shape=(40, 40, 3), widths=(8, 16, 32, 64),
                 augmentation=[L.RandomCrop(32, 32), L.RandomFlip()])
    assert NativeGraphEngine.layers_eligible(m) == (True, "")
    p = NativeGraphEngine.plan_only(m, 8)
    assert p.cin_pad == 4 and p.x0.shape == (8, 40, 40, 4)
    assert p.nodes[0].kind == "Augment" and p.nodes[0].out.shape == (8, 32, 32, 4)
    assert sum(nd.kind == "Augment" for nd in p.nodes) == 1
    plain = NativeGraphEngine.plan_only(resnet18(10, input_shape=(32, 32, 3), widths=(8, 16, 32, 64)), 8)
    assert [nd.kind for nd in p.nodes[1:]] == [nd.kind for nd in plain.nodes]
    assert {k: v for k, v in p.describe_plan().items() if k not in ("nodes", "kernels_fwd")} == \
        {k: v for k, v in plain.describe_plan().items() if k not in ("nodes", "kernels_fwd")}


def test_fallback_reasons():
    st = _FakeGPUStrategy()
    for late in (L.RandomFlip(), L.RandomCrop(8, 8), L.ZeroPadding2D(1)):
        m = keras.Sequential([L.Conv2D(8, 3, padding="same", input_shape=(8, 8, 3)), late, L.Flatten(), L.Dense(4)])
        m.compile(optimizer="sgd", loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
        why = f"layer {type(late).__name__} is native only ahead of the first weight layer"
        assert NativeGraphEngine.eligible(m, st) == (False, why)
        assert NativeInference.eligible(m, "cuda") == (False, why)
    # a prefix layer whose input is read twice is not part of the prefix
    inp = L.Input((8, 8, 3))
    a, b = L.RandomFlip()(inp), L.Conv2D(8, 3, padding="same")(inp)
    fm = keras.Model(inp, L.Dense(4)(L.Flatten()(L.Add()([L.Conv2D(8, 3, padding="same")(a), b]))))
    assert NativeGraphEngine.layers_eligible(fm) == (False,
                                                     "layer RandomFlip is native only ahead of the first weight layer")
    nine = [L.RandomFlip(input_shape=(8, 8, 3))] + [L.RandomFlip() for _ in range(8)]
    m9 = keras.Sequential(nine + [L.Conv2D(8, 3, padding="same"), L.Flatten(), L.Dense(4)])
    ok, why = NativeGraphEngine.layers_eligible(m9)
    assert not ok and "9" in why and f"AUG_MAX_STAGES = {H.AUG_MAX_STAGES}" in why and H.AUG_MAX_STAGES == 8
    m8 = keras.Sequential(nine[:8] + [L.Conv2D(8, 3, padding="same"), L.Flatten(), L.Dense(4)])
    assert NativeGraphEngine.layers_eligible(m8) == (True, "")
    assert len(NativeGraphEngine.plan_only(m8, 2).nodes[0].attrs["stages"]) == 8
    with pytest.raises(ValueError):
        H.aug_table([(H.AUG_FLIP, 3, 0, 0, 0, 1)] * 9)


def test_plans_without_a_prefix_are_unchanged():
    p = NativeGraphEngine.plan_only(_cifar_net(prefix=False), 8)
    assert [nd.kind for nd in p.nodes] == ["Conv2D", "MaxPooling2D", "Flatten", "Dense"]
    assert p.nodes[0].inputs == [p.x0] and p.x0.consumers == [p.nodes[0]]
    r = NativeGraphEngine.plan_only(resnet18(), 8)
    assert not any(nd.kind == "Augment" for nd in r.nodes) and r.describe_plan()["nodes"] == 68
    assert r.cin_pad == 4 and r.x0.shape == (8, 224, 224, 4)


# --- 6. the generic engine -----------------------------------------------------------------------------
def _fit_steps(m, x, y, steps, initial_epoch=0):
    m.fit(x, y, batch_size=8, epochs=initial_epoch + 1, initial_epoch=initial_epoch, steps_per_epoch=steps,
          shuffle=False, verbose=0)
    return m.get_weights()


def test_generic_engine_augments_and_resumes(tmp_path):
    rng = np.random.default_rng(3)
    x, y = rng.random((16, 16, 16, 3)).astype(np.float32), rng.integers(0, 10, 16)
    a = _cifar_net()
    w0 = a.get_weights()
    # 2 steps of 8 rows == 1 step on rows 0..7 at t = 1 and 1 step on rows 0..7 at t = 2 ... so
    # compare with a prefix-less model fed the oracle's batches, one step (one epoch) each
    wa = _fit_steps(a, x[:8], y[:8], 1)
    assert a._engine.name == "generic" and int(a.optimizer.iterations) == 1
    stages, _, _ = H.aug_stages(a.layers[:3], L.augment_seeds(a), 16, 16)
    b = _cifar_net(prefix=False)
    b.set_weights(w0)
    wb = _fit_steps(b, H.augment_reference(x[:8], stages, 1, 0, True), y[:8], 1)
    assert all(np.array_equal(p, q) for p, q in zip(wa, wb))
    assert not np.array_equal(H.augment_reference(x[:8], stages, 1, 0, True), x[:8])
    # resume: 2 steps, save / load, 2 more == 4 steps
    c = _cifar_net()
    c.set_weights(w0)
    w4 = _fit_steps(c, np.concatenate([x, x]), np.concatenate([y, y]), 4)
    d = _cifar_net()
    d.set_weights(w0)
    _fit_steps(d, x, y, 2)
    path = str(tmp_path / "ck.h5")
    d.save(path)
    e = keras.models.load_model(path)
    assert int(e.optimizer.iterations) == 2
    wr = _fit_steps(e, x, y, 2)
    assert int(e.optimizer.iterations) == 4
    assert all(np.array_equal(p, q) for p, q in zip(w4, wr))
    # ... and the second pair of steps did not repeat the first pair's transforms
    f = _cifar_net()
    f.set_weights(d.get_weights())
    f.optimizer.iterations = 0
    assert not all(np.array_equal(p, q) for p, q in zip(_fit_steps(f, x, y, 2), wr))


@pytest.mark.dist
@pytest.mark.timeout(300)
def test_world_2_matches_world_1(tmp_path):
    def run(world, per):
        d = tmp_path / f"w{world}"
        d.mkdir()
        env = {"DAMD_DEVICE": "cpu", "DAMD_TEST_OUT": str(d), "PYTHONPATH": ROOT, "OMP_NUM_THREADS": "2",
               "DAMD_LOG_LEVEL": "WARNING", "DAMD_TEST_PER_REPLICA": str(per)}
        res = launch.launch_script([WORKER], nproc=world, env=env, timeout=240)
        assert res.ok, res.returncodes
        out = []
        for r in range(world):
            w = dict(np.load(os.path.join(d, f"rank{r}.npz")))
            with open(os.path.join(d, f"rank{r}.json")) as f:
                out.append((w, json.load(f)))
        return out

    (w0, j0), (w1, j1) = run(2, 4)
    ((ws, js),) = run(1, 8)
    assert j0["world"] == 2 and js["world"] == 1 and j0["engine"] == js["engine"] == "generic"
    assert j0["iterations"] == js["iterations"] == 2
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k  # replicas stay bitwise mirrored
        # the tolerances of the clipping / regularizer world-2 versus world-1 comparisons (the
        # exchange sums the replicas' gradients in another order than one replica sums its rows)
        np.testing.assert_allclose(w0[k], ws[k], rtol=1e-4, atol=1e-6, err_msg=k)
    np.testing.assert_allclose(j0["loss"], js["loss"], rtol=1e-5)
