"""The split-K plans of ops/hip.py, frozen row by row (tests/golden/splitk_plans.json).

The planners are pure arithmetic on shapes and a few knobs, and every plan fixes a summation
order, so a changed plan changes bits and workspace sizes.  The table below puts shapes on both
sides of every branch of the planners (test_table_covers_every_branch asserts that it does) and
test_plans_equal_golden compares each row with the golden for exact equality.  CPU only: no
native module is called.

    python tests/test_splitk_plans.py --write   # records tests/golden/splitk_plans.json

Record only at the parent commit of a change to the planners, never with the code under test."""
from __future__ import annotations

import contextlib
import json
import os
import sys
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from distributed_amd.ops import hip as H  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "splitk_plans.json")

# the planners' knobs: module globals of hip (read from the environment at import; pinned here
# so the table does not depend on the caller's environment) and variables read per call
GLOBALS = {"SPLIT_MIN_TILES": 320, "SPLIT_TARGET_WG": 384, "WGRAD_TARGET_WG": 512, "WGRAD_SLAB_MAX": 64 << 20,
           "DENSE_SPLIT_MAX_TILES": 32, "DENSE_SPLIT_TARGET_WG": 128}
ENV = ("DAMD_CONV_KB", "DAMD_CONV_GLDS", "DAMD_WGRAD_KERNEL", "DAMD_WGRAD3_WG", "DAMD_CONV3", "DAMD_CONV3_MIN_WG",
       "DAMD_DGRAD_SUBPIX")


@contextlib.contextmanager
def knobs(setting: str):
    """``setting``: "" or "NAME=value[,NAME=value]"; a DAMD_* name is an environment variable,
    any other a global of hip."""
    pairs = [p.split("=") for p in setting.split(",") if p]
    env = {k: v for k, v in pairs if k.startswith("DAMD_")}
    glob = dict(GLOBALS, **{k: int(v) for k, v in pairs if not k.startswith("DAMD_")})
    assert set(glob) == set(GLOBALS) and set(env) <= set(ENV), setting
    with mock.patch.dict(os.environ), mock.patch.multiple(H, **glob):
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield


# ---- GEMM rows: (M, N, K) ------------------------------------------------------------------
GEMM_M = (64, 257, 4097, 12544, 200704)
GEMM_N = (16, 64, 72, 200, 1000)
GEMM_K = (63, 64, 255, 256, 257, 480, 481, 511, 512, 513, 50176)
GEMM_EXTRA = [
    # the classifier (batch 64, 512 -> 1000) and its transposes; the MNIST CNN's dense layers
    (64, 1000, 512), (64, 512, 1000), (512, 1000, 64), (1000, 512, 64), (512, 64, 1000), (1000, 64, 512),
    (64, 1008, 512), (512, 1008, 64), (64, 64, 5408), (64, 5408, 64), (5408, 64, 64), (64, 16, 64), (64, 64, 16),
    (64, 16, 5408),
    # the dense gate: 32 | 33 tiles of 128 x 128 and of 256 x 64, K = 63 | 64
    (4096, 128, 63), (4096, 128, 64), (4097, 128, 64), (4096, 128, 512), (4097, 128, 512),
    (8192, 64, 63), (8192, 64, 64), (8193, 64, 64), (8192, 64, 512), (8193, 64, 512),
    # split_plan's gate: 319 | 320 tiles
    (40832, 128, 2304), (40833, 128, 2304), (40960, 128, 2304), (81664, 64, 2304), (81665, 64, 2304),
    (40832, 64, 1152), (20416, 128, 1152), (20417, 128, 1152),
    # the dense weight gradient: one slab (few tiles, >= 32 K elements), atomic, several slabs
    (512, 1000, 256), (512, 1000, 512), (512, 24, 64), (512, 24, 40), (24, 40, 512), (24, 40, 511), (24, 40, 1024),
    (128, 256, 64), (128, 255, 64), (1024, 1024, 64), (1152, 1024, 64),
    # ResNet-18 layer GEMMs (batch 64): M = pixels, K = taps x channels
    (200704, 64, 576), (50176, 128, 1152), (12544, 256, 2304), (3136, 512, 4608), (3136, 512, 2304),
    (3136, 256, 4608), (50176, 128, 64), (12544, 256, 128), (3136, 512, 256), (802816, 64, 224),
]
GEMM_KNOB_ROWS = [(64, 1000, 512), (512, 1000, 64), (3136, 512, 4608), (12544, 256, 2304), (50176, 128, 1152),
                  (200704, 512, 513), (4096, 1024, 4096), (257, 200, 1000), (576, 64, 200704), (24, 40, 512)]
GEMM_KNOBS = ("SPLIT_MIN_TILES=0", "SPLIT_MIN_TILES=1073741824", "WGRAD_TARGET_WG=1", "WGRAD_TARGET_WG=65536",
              "WGRAD_SLAB_MAX=4194304", "SPLIT_TARGET_WG=65536,SPLIT_MIN_TILES=1073741824", "DENSE_SPLIT_TARGET_WG=1",
              "DENSE_SPLIT_MAX_TILES=1024")


def gemm_rows():
    shapes = dict.fromkeys([(m, n, k) for m in GEMM_M for n in GEMM_N for k in GEMM_K] + GEMM_EXTRA)
    return [(s, "") for s in shapes] + [(s, kn) for kn in GEMM_KNOBS for s in GEMM_KNOB_ROWS]


def gemm_eval(M, N, K):
    """dense_split_plan (2 values), dense_workspace_elems, wgrad_plan (3), wgrad_workspace_elems,
    split_plan (2 each) at (tile 0, bk 32), (0, 64), (1, 32), (1, 64), as one flat list."""
    return [*H.dense_split_plan(M, N, K), H.dense_workspace_elems(M, N, K), *H.wgrad_plan(M, N, K),
            H.wgrad_workspace_elems(M, N, K),
            *(v for t in (0, 1) for bk in (32, 64) for v in H.split_plan(M, N, K, t, bk))]


# ---- conv rows: (n, hw, cin, cout, k, stride, padding) ------------------------------------
CONV_GRID = [(n, hw, cin, cout, k, s, pad)
             for n in (2, 64)
             for hw in (7, 14, 16, 17, 56, 62, 140)
             for cin, cout in ((8, 16), (16, 64), (64, 128), (128, 72), (256, 512))
             for k, s, pad in ((3, 1, "same"), (3, 2, "same"), (1, 2, "valid"))]
RESNET18 = [  # distributed_amd/models/resnet.py at batch 64 (the stem's 3 input channels padded to 4)
    (64, 224, 4, 64, 7, 2, "same"),
    (64, 56, 64, 64, 3, 1, "same"),
    (64, 56, 64, 128, 3, 2, "same"), (64, 28, 128, 128, 3, 1, "same"), (64, 56, 64, 128, 1, 2, "valid"),
    (64, 28, 128, 256, 3, 2, "same"), (64, 14, 256, 256, 3, 1, "same"), (64, 28, 128, 256, 1, 2, "valid"),
    (64, 14, 256, 512, 3, 2, "same"), (64, 7, 512, 512, 3, 1, "same"), (64, 14, 256, 512, 1, 2, "valid"),
]
MNIST = [(64, 28, 8, 32, 3, 1, "valid"), (64, 13, 32, 64, 3, 1, "valid"), (256, 28, 8, 32, 3, 1, "valid")]
CONV_EXTRA = [
    # packed-tap stems (Cin 4, even stride): 7x7 / 5x5 / 3x3, split and unsplit forward plans
    (2, 32, 4, 16, 7, 2, "same"), (32, 32, 4, 16, 7, 2, "same"), (8, 64, 4, 64, 7, 2, "same"),
    (1, 224, 4, 64, 7, 2, "same"), (16, 224, 4, 64, 7, 2, "same"), (256, 224, 4, 64, 7, 2, "same"),
    (8, 32, 4, 32, 3, 2, "same"), (8, 32, 4, 32, 5, 2, "same"), (8, 33, 4, 32, 7, 2, "same"),
    (8, 32, 4, 12, 7, 2, "same"),
    # several segments per image row (Wo > 64), N <= 64 and N > 64
    (1, 140, 8, 16, 3, 1, "same"), (1, 140, 8, 128, 3, 1, "same"), (4, 130, 64, 128, 3, 1, "valid"),
    # n x ho x nseg >= 2^21 virtual rows: back to the register-staged kernel
    (5000, 140, 8, 128, 3, 1, "same"), (4993, 140, 8, 128, 3, 1, "same"), (37450, 56, 8, 128, 3, 1, "same"),
    # 5x5: odd padding at stride 2 (no sub-pixel dgrad), a long K
    (8, 56, 64, 64, 5, 2, "same"), (8, 56, 64, 128, 5, 1, "same"), (8, 28, 128, 128, 5, 2, "same"),
    # direct 3x3 at the edges of its shape rules: W 62 | 63, few blocks, 192 channels
    (8, 62, 64, 64, 3, 1, "same"), (8, 63, 64, 64, 3, 1, "same"), (1, 8, 64, 64, 3, 1, "same"),
    (16, 32, 192, 192, 3, 1, "same"), (512, 8, 64, 64, 3, 1, "same"), (300, 62, 128, 64, 3, 1, "same"),
    (1, 56, 512, 512, 3, 1, "same"), (8, 16, 64, 64, 3, 1, "same"), (8, 16, 64, 128, 3, 1, "same"),
    # small ResNets of the tests and smoke(): widths 16 / 32 / 64 on 32 x 32 images
    (32, 32, 4, 16, 7, 2, "same"), (32, 8, 16, 16, 3, 1, "same"), (32, 8, 16, 32, 3, 2, "same"),
    (32, 4, 32, 32, 3, 1, "same"), (32, 4, 32, 64, 3, 2, "same"), (32, 2, 64, 64, 3, 1, "same"),
    (32, 8, 16, 32, 1, 2, "valid"),
]
CONV_KNOB_ROWS = RESNET18[:3] + RESNET18[8:10] + MNIST[:1] + [
    (2, 32, 4, 16, 7, 2, "same"), (8, 64, 4, 64, 7, 2, "same"), (1, 140, 8, 16, 3, 1, "same"),
    (1, 140, 8, 128, 3, 1, "same"), (5000, 140, 8, 128, 3, 1, "same"), (8, 16, 64, 64, 3, 1, "same"),
    (8, 17, 64, 128, 3, 1, "same"), (2, 62, 64, 64, 3, 1, "same"), (8, 56, 64, 64, 5, 2, "same"),
]
CONV_KNOBS = ("WGRAD_TARGET_WG=1", "DAMD_CONV_KB=32", "DAMD_CONV_GLDS=0", "DAMD_WGRAD_KERNEL=direct",
              "DAMD_WGRAD_KERNEL=glds", "DAMD_WGRAD_KERNEL=reg", "DAMD_WGRAD3_WG=64", "SPLIT_MIN_TILES=0",
              "SPLIT_MIN_TILES=1073741824", "WGRAD_SLAB_MAX=4194304", "WGRAD_TARGET_WG=65536",
              "DAMD_WGRAD_KERNEL=glds,DAMD_CONV_KB=32", "DAMD_WGRAD_KERNEL=glds,WGRAD_TARGET_WG=1",
              "DAMD_CONV3_MIN_WG=1", "DAMD_CONV3=0", "DAMD_DGRAD_SUBPIX=0")


def conv_rows():
    return ([(c, "") for c in dict.fromkeys(CONV_GRID + RESNET18 + MNIST + CONV_EXTRA)]
            + [(c, kn) for kn in CONV_KNOBS for c in CONV_KNOB_ROWS])


def conv_args(n, hw, cin, cout, k, s, pad):
    return (n, hw, hw, cin), (k, k, cin, cout), (s, s), pad


PLAN_KEYS = ("amode", "M", "N", "K", "tile", "splits", "kps", "kstep", "stats_T", "ws")


def plan_values(plan: dict) -> list:
    """The whole plan dict as its values in PLAN_KEYS order (None: the plan has no such key)."""
    assert set(plan) <= set(PLAN_KEYS) and None not in plan.values(), plan
    return [plan.get(k) for k in PLAN_KEYS]


def conv_eval(*conv):
    """[conv_fwd_plan, conv_dgrad_plan, conv_wgrad_plan (plan_values each), conv_wgrad_workspace_elems]"""
    a = conv_args(*conv)
    return [plan_values(H.conv_fwd_plan(*a)), plan_values(H.conv_dgrad_plan(*a)), plan_values(H.conv_wgrad_plan(*a)),
            H.conv_wgrad_workspace_elems(*a)]


def row_key(kind, shape, setting):
    return f"{kind} {'x'.join(map(str, shape))}" + (f" | {setting}" if setting else "")


def table() -> dict:
    """key -> plans of every row, in JSON's types (lists for tuples)."""
    out = {}
    for kind, rows, fn in (("gemm", gemm_rows(), gemm_eval), ("conv", conv_rows(), conv_eval)):
        for shape, setting in rows:
            with knobs(setting):
                val = fn(*shape)
            key = row_key(kind, shape, setting)
            assert key not in out, f"duplicate row {key}"
            out[key] = json.loads(json.dumps(val))
    return out


def write_golden():
    rows = table()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}"
                                  for k, v in rows.items()) + "\n}\n")
    print(f"wrote {len(rows)} rows to {GOLDEN}")


def test_plans_equal_golden():
    with open(GOLDEN) as f:
        golden = json.load(f)
    rows = table()
    assert list(rows) == list(golden), "the table's rows are not the golden's rows"
    wrong = [k for k in rows if rows[k] != golden[k]]
    assert not wrong, f"{len(wrong)} of {len(rows)} plans differ, first: {wrong[0]}: {rows[wrong[0]]} != " \
                      f"golden {golden[wrong[0]]}"
    assert 800 <= len(rows) <= 4000


def _tiles(M, N, tile):
    bm, bn = (256, 64) if tile == 1 else (128, 128)
    return -(-M // bm) * -(-N // bn)


def test_table_covers_every_branch():
    """Each kind of row the planners branch on occurs at least once (so the table cannot lose a
    branch unnoticed); the conditions are recomputed here from the shapes."""
    seen = set()
    for (M, N, K), setting in gemm_rows():
        with knobs(setting):
            t = H.pick_tile(N)
            seen.add(f"tile{t}")
            if M % 128 and N % 64 and N % 128:
                seen.add("ragged")
            for tile in (0, 1):
                side = "split-gate-closed" if _tiles(M, N, tile) >= H.SPLIT_MIN_TILES else "split-gate-open"
                seen.add(f"{side}-tile{tile}")
                if _tiles(M, N, tile) in (H.SPLIT_MIN_TILES - 1, H.SPLIT_MIN_TILES):
                    seen.add(f"split-gate-edge-{_tiles(M, N, tile) - H.SPLIT_MIN_TILES}")
            seen.add(f"K{K}")
            if K % 64 and K % 32:
                seen.add("K-ragged")
            cap = H.WGRAD_SLAB_MAX // (M * N * 4)
            tiles = _tiles(M, N, t)
            if max(1, cap) < min(-(-H.WGRAD_TARGET_WG // tiles), max(1, K // 256)):
                seen.add("slab-cap-bites")
            if cap == 0:
                seen.add("slab-larger-than-cap")
            seen.add(f"dense-tiles{tiles}" if tiles in (32, 33) else "dense-tiles-other")
            seen.add("dense-" + ("split" if H.dense_split_plan(M, N, K)[0] > 1 else "unsplit"))
            ws, (_, splits, _) = H.wgrad_workspace_elems(M, N, K), H.wgrad_plan(M, N, K)
            seen.add("dense-wgrad-" + ("atomic" if ws == 0 else "slab1" if splits == 1 else "slabs"))
        seen.add(setting.split("=")[0])
    assert {(64, 1000, 512), (64, 512, 1000), (512, 1000, 64)} <= {s for s, _ in gemm_rows()}
    for conv, setting in conv_rows():
        n, hw, cin, cout, k, s, pad = conv
        with knobs(setting):
            a = conv_args(*conv)
            fwd, dg, wg = H.conv_fwd_plan(*a), H.conv_dgrad_plan(*a), H.conv_wgrad_plan(*a)
            wo = H.conv_out(hw, k, s, pad)[0]
            stem = H.stem4_ok(*a)
        seen.add(f"fwd-amode{fwd['amode']}-" + ("split" if fwd["splits"] > 1 else "unsplit"))
        seen.add(f"dgrad-amode{dg['amode']}-" + ("split" if dg["splits"] > 1 else "unsplit"))
        if dg["amode"] == H.A_DGRAD64 and s == 2:
            seen.add("dgrad-subpixel")
        seen.add(f"wgrad-amode{wg['amode']}-" + ("split" if wg["splits"] > 1 else "unsplit"))
        if stem:
            seen.add("stem")
            if (cin, k, s, pad) == (4, 7, 2, "same"):
                seen.add("stem-7x7")
        if wg["amode"] == H.A_WGRAD64 and not stem:
            seen.add(f"wgrad64-kstep{wg['kstep']}-" + ("narrow" if wo <= 16 else "wide"))
            if wo > 64:
                seen.add("wgrad64-segments")
        if wg["amode"] == H.A_WGRAD and cout <= 64:
            seen.add("wgrad-reg-narrow")
        if wg["amode"] == H.A_WGRAD and cout > 64 and not setting and n * wo * -(-wo // 64) >= 1 << 21:
            seen.add("wgrad-2^21-fallback")
        if wg["amode"] == H.A_WGRAD3:
            assert cin % 64 == 0 and cout % 64 == 0 and hw <= 62
        for part in setting.split(","):
            seen.add(part)
    need = {
        "tile0", "tile1", "ragged", "K-ragged", "slab-cap-bites", "slab-larger-than-cap",
        "split-gate-open-tile0", "split-gate-closed-tile0", "split-gate-open-tile1", "split-gate-closed-tile1",
        "split-gate-edge--1", "split-gate-edge-0", "SPLIT_MIN_TILES=0", "SPLIT_MIN_TILES=1073741824",
        "dense-tiles32", "dense-tiles33", "dense-split", "dense-unsplit",
        "dense-wgrad-atomic", "dense-wgrad-slab1", "dense-wgrad-slabs",
        "stem", "stem-7x7", "wgrad-reg-narrow", "wgrad-2^21-fallback", "wgrad64-segments", "dgrad-subpixel",
        "wgrad64-kstep32-narrow", "wgrad64-kstep64-wide",
        "WGRAD_TARGET_WG=1", "DAMD_CONV_KB=32", "DAMD_CONV_GLDS=0", "DAMD_WGRAD_KERNEL=direct",
        "DAMD_WGRAD_KERNEL=glds", "DAMD_WGRAD_KERNEL=reg", "DAMD_WGRAD3_WG=64",
    }
    need |= {f"K{k}" for k in (63, 64, 255, 256, 257, 480, 481, 511, 512, 513)}
    for amode, name in ((H.A_CONV64, "fwd"), (H.A_IM2COL, "fwd"), (H.A_DGRAD64, "dgrad"), (H.A_DGRAD, "dgrad"),
                        (H.A_WGRAD64, "wgrad"), (H.A_WGRAD3, "wgrad"), (H.A_WGRAD, "wgrad")):
        need |= {f"{name}-amode{amode}-split", f"{name}-amode{amode}-unsplit"}
    need |= {f"fwd-amode{H.A_CONV3}-unsplit", f"dgrad-amode{H.A_DGRAD3}-unsplit"}
    assert not need - seen, sorted(need - seen)
    for conv in RESNET18 + MNIST[:2]:
        assert (conv, "") in conv_rows()


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_splitk_plans.py --write")
    write_golden()
