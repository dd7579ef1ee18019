"""Phase-stamp diagnostics of the fused ConvNet step (DAMD_STAMPS=1).

Runs warm steps, then one more step, and prints per kernel / per phase the median
(over blocks) time since that kernel's earliest block start, in microseconds
(s_memrealtime ticks at 100 MHz)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["DAMD_STAMPS"] = "1"
os.environ.setdefault("DAMD_GRAPH", "1")
os.environ.setdefault("DAMD_GRAPH_STEPS", "10")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import distributed_amd as tf  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    (x, y), _ = tf.keras.datasets.mnist.load_data()
    x = x.reshape(len(x), 28, 28, 1) / 255.0
    m = tf.models.mnist_cnn()
    tf.models.compile_reference(m)
    eng = m._get_engine(B, B)
    eng.bind(x, y)
    eng.start_epoch(0, True, wrap_steps=len(x) // B)
    eng.run(50)
    eng.sync()
    eng.stamps.zero_()
    eng.run(10)  # one captured 10-step graph; the stamps keep the last step's values
    eng.sync()
    st = eng.stamps.cpu().numpy()
    NS = eng.trainer.num_slices
    # a role per block in the flagship backward (CfgFlagBwd::SPLIT): blocks 0 .. NSB - 1 are the
    # conv role, NSB .. 2 NSB - 1 the W1 role; both are reported against the kernel's first block
    NSB, nblk = eng.trainer.num_slices_bwd, eng.trainer.bwd_blocks
    grids = {"fwd": (0, 0, NS * ((B + 15) // 16))}
    if nblk == 2 * NSB:
        grids["bwd conv role"] = (2, 0, NSB)
        grids["bwd W1 role"] = (2, NSB, 2 * NSB)
    else:
        grids["bwd"] = (2, 0, nblk)
    names = {"fwd": ["start", "loads+sgd", "xs staged", "conv done", "atomics issued", "conv setup", "conv pool",
                     "pooled/code out", "dense-1 mfma", "dense-1 barrier"],
             "bwd": ["start", "loads staged", "head done", "mfma", "convgrad", "end", "h", "softmax", "dh",
                     "logit operands", "logit mfma+max/sum", "lse/argmax", "w0 softmax stored",
                     "w4 body stored"]}
    names["bwd conv role"] = names["bwd"]
    # the W1 role has no dP / conv gradient: slot 3 is stamped once its update stores are issued,
    # slot 4 behind its aux sums
    names["bwd W1 role"] = [{"mfma": "update stored", "convgrad": "aux sums"}.get(nm, nm) for nm in names["bwd"]]
    t0 = None
    for kn, (k, lo, hi) in grids.items():
        a = st[k, lo:hi].astype(np.int64)
        n = hi - lo
        # (the roles share one launch: both against the launch's earliest block)
        allb = st[k, :(nblk if k == 2 else hi), 0].astype(np.int64)
        base = allb[allb > 0].min()
        t0 = base if t0 is None else t0
        own = a[:, 0][a[:, 0] > 0]
        print(f"{kn}: {n} blocks, first block of the launch at +{(base - t0) / 100:.2f} us, these blocks start "
              f"median +{statistics.median((own - base) / 100.0):.2f} max +{(own.max() - base) / 100:.2f} us")
        for j, nm in enumerate(names[kn]):
            col = a[:, j]
            col = col[col > 0]
            if len(col) == 0:
                continue
            d = (col - base) / 100.0
            print(f"   {j} {nm:14s} median {statistics.median(d):7.2f}  min {d.min():7.2f}  max {d.max():7.2f} us")
        if kn == "fwd":
            per_wave(a)
        elif kn != "bwd W1 role":  # (slot 15 is the conv role's pre-conv-gradient barrier)
            # the recorded wave's arrival at the barrier ahead of the `red` reduction: block b's
            # value is slot b & 15 of row nblk + (b >> 4), behind the rows of the grid
            red = st[k, nblk:].astype(np.int64).reshape(-1)[lo:hi]
            per_wave_bwd(a, red)


def per_wave_bwd(a, red):
    """bwd slots 14 / 15: block s records the view of wave s mod NW -- its arrival at the dh
    barrier and at the pre-conv-gradient barrier (wave 0 records the time it LEAVES them in
    slots 8 and 3).  The top byte of slot 14 is the wave, of slot 15 the waves per block.
    red: per block, the same wave's arrival at the barrier ahead of the `red` reduction, i.e. the
    end of its conv gradient (wave 0's own arrival is slot 4, 'convgrad').
    Medians over the blocks that recorded the wave, in us since the block's own start; then the
    conv gradient's span: pre-conv-gradient barrier left (slot 3) to the last recorded arrival."""
    mask = (1 << 56) - 1
    ok = (a[:, 15] != 0) & (a[:, 0] > 0)
    if not ok.any():
        return
    nw = int(a[ok][0, 15] >> 56)
    wave = a[:, 14] >> 56
    print(f"bwd per wave ({nw} waves per block; median us since the block's own start of the wave's ARRIVAL at the barrier;")
    print("   '0 leaves': when wave 0 leaves it, i.e. after the last arrival)")
    print("   wave  blocks  dh barrier  pre-conv-grad barrier  red barrier  conv gradient (from slot 3)")
    rows = a[ok]
    print(f"   0 leaves {len(rows):3d}  {statistics.median((rows[:, 8] - rows[:, 0]) / 100.0):10.2f}  "
          f"{statistics.median((rows[:, 3] - rows[:, 0]) / 100.0):21.2f}")
    has_red = ok & ((red & mask) > 0)
    span = {}
    for w in range(nw):
        sel = ok & (wave == w)
        rows = a[sel]
        if len(rows):
            d = [statistics.median(((rows[:, s] & mask) - rows[:, 0]) / 100.0) for s in (14, 15)]
            line = f"   {w:4d}  {len(rows):6d}  {d[0]:10.2f}  {d[1]:21.2f}"
            rsel = sel & has_red
            if rsel.any():
                r = red[rsel] & mask
                span[w] = statistics.median((r - a[rsel][:, 3]) / 100.0)
                line += f"  {statistics.median((r - a[rsel][:, 0]) / 100.0):11.2f}  {span[w]:13.2f}"
            print(line)
    if span:
        w0 = a[has_red]
        print(f"   conv gradient: wave 0 alone (slot 4 - slot 3) median {statistics.median((w0[:, 4] - w0[:, 3]) / 100.0):.2f} us; "
              f"to the last wave's arrival (largest per-wave median, wave {max(span, key=span.get)}) {max(span.values()):.2f} us")


def per_wave(a):
    """fwd slots 10-14: block lin records the view of wave lin mod NW (slot 14: wave | NW << 8)
    of the phases wave 0 records in slots 5, 6, 8 and 4.  Medians over the blocks that
    recorded the wave, in us since the block's OWN start (slot 0), so blocks that start late
    do not blur the comparison between waves."""
    tag = a[:, 14]
    ok = (tag > 0) & (a[:, 0] > 0)
    if not ok.any():
        return
    nw = int(tag[ok][0] >> 8)
    names = ["conv setup", "conv pool", "dense-1 mfma", "atomics issued"]
    print(f"fwd per wave ({nw} waves per block; median us since the block's own start; 'conv pool' = arrival at the")
    print("   post-conv barrier, 'dense-1 mfma' = arrival at the dense-1 barrier or, without one, end of the wave's tile / stores)")
    print("   wave  blocks  " + "  ".join(f"{nm:>14s}" for nm in names))

    def line(label, rows, slots):
        med = [statistics.median((rows[:, s] - rows[:, 0]) / 100.0) if (rows[:, s] > 0).all() else float("nan")
               for s in slots]
        print(f"   {label:>4s}  {len(rows):6d}  " + "  ".join(f"{m:14.2f}" for m in med))

    line("0*", a[ok], (5, 6, 8, 4))  # wave 0 as every block records it
    for w in range(nw):
        rows = a[ok & ((tag & 0xff) == w)]
        if len(rows):
            line(str(w), rows, (10, 11, 12, 13))
    late = a[ok]
    d = (late[:, 3] - late[:, 6]) / 100.0
    print(f"   wave 0's wait at the post-conv barrier (slot 3 - slot 6): median {statistics.median(d):.2f} us")


if __name__ == "__main__":
    main()
