"""The fused MNIST step's model constants and device buffers (csrc/include/convnet.h
ConvNetBuffers), as ``ConvNetTrainer`` (csrc/bindings.cpp) takes them.

One allocation sequence for the engine, the exchange self-test's scratch trainers and the
in-process multi-rank test, in an order kept on purpose (see ``w1bf_bufs``).
"""
import torch

from .ctrl import WORDS

NPARAM = 347146
NGRAD = 347152  # + padding; the [loss, correct, count] metric tail sits at NPARAM
HID, NCLS, FEAT, NCONV = 64, 10, 5408, 320
SHAPES = [(3, 3, 1, 32), (32,), (5408, 64), (64,), (64, 10), (10,)]  # Keras weight order
OFF_W1, OFF_B1 = NCONV, NCONV + FEAT * HID  # W1 inside the flat parameter vector


def exchange_capacity(C, world: int, PP: int, ppb: int, sharded: bool) -> int:
    """Staging floats of the sharded in-kernel exchange (convnet.h XArgs) at ``world`` ranks, or of
    the standalone peer all-reduce of the gradient + conv sums."""
    if not sharded:
        return C.PeerAllreduce.message_words(C.convnet_grad_count(PP), 2 * NCONV)
    NU = 4 * C.convnet_num_slices(ppb)
    return max(world * NU * 2048, 347648 + 2 * 8 * 1408 + 16384 + FEAT * HID // 2)


class ConvNetBuffers:
    """What one ConvNetTrainer at per-replica batch ``B`` trains in.  ``P0``: the parameters
    start as a clone of it (else zero).  ``parity_w1bf``: two zeroed bf16 W1 buffers, one per
    step parity (else one copy made from P).  ``prefetch``: the next-batch quartet."""

    def __init__(self, C, dev, B, PP, P0=None, parity_w1bf=False, prefetch=False):
        self.device = dev
        f32 = dict(dtype=torch.float32, device=dev)
        BP = (B + 63) // 64 * 64  # padded batch pitch of the feature-major buffers
        self.P = torch.zeros(NGRAD, **f32) if P0 is None else P0.clone()
        self.G = torch.zeros(C.convnet_grad_count(PP), **f32)  # grads + metric tail
        self.V = torch.zeros(NGRAD, **f32)
        self.ctrl = torch.zeros(WORDS, dtype=torch.int32, device=dev)
        self.w1alt = torch.zeros(FEAT * HID, **f32)   # W1 double buffer (by step parity)
        self.v1alt = torch.zeros(FEAT * HID, **f32)
        # bf16 copy of W1, one buffer per step parity: a step reads the buffer of its parity,
        # the eager update in bwd writes the other one (convnet.h).
        # Two allocations of 0.7 MB, not one of 1.4 MB: as one tensor (a request above 1 MB,
        # which the caching allocator serves from other segments) the forward kernel measured
        # 0.4 us longer; why was not established (BENCH.md, round 11)
        if parity_w1bf:
            self.w1bf_bufs = tuple(torch.zeros(FEAT * HID, dtype=torch.bfloat16, device=dev) for _ in range(2))
        else:
            self.w1bf_bufs = (self.P[OFF_W1:OFF_B1].to(torch.bfloat16),)
        self.pooled = torch.zeros(FEAT, BP, dtype=torch.bfloat16, device=dev)
        self.code = torch.zeros(B, FEAT, dtype=torch.uint8, device=dev)
        self.hacc = torch.zeros(C.convnet_hacc_elems(B), dtype=torch.int64, device=dev)  # by step parity
        self.hconv = torch.zeros(2 * NCONV, dtype=torch.int64, device=dev)
        self.calt = torch.zeros(2 * NCONV, **f32)  # alternate conv parameters + velocity
        # next-batch prefetch: bwd copies the next step's rows here for the next fwd, tagged
        # with the ctrl block's data generation + cursor
        self.xnext = self.xtag = self.xcur = self.ycur = None
        if prefetch:
            self.xnext = torch.zeros(B * 784, **f32)  # (u8 rows use the first quarter)
            self.xtag = torch.zeros(1, dtype=torch.int64, device=dev)
            # this step's rows / labels as the fwd read them, for the bwd (no cursor needed)
            self.xcur = torch.zeros(B * 784, **f32)
            self.ycur = torch.zeros(B, dtype=torch.int32, device=dev)
        self.stamps = None

    def trainer_args(self, ppb: int, eager_w1: int = 0, specialised=None) -> dict:
        """The ``bufs`` dict of ConvNetTrainer (its keys: csrc/bindings.cpp).  ``specialised``
        None: the key is not passed."""
        ptr = {k: t.data_ptr() for k, t in dict(
            params=self.P, grads=self.G, velocity=self.V, ctrl=self.ctrl, pooled=self.pooled, code=self.code,
            w1alt=self.w1alt, v1alt=self.v1alt, w1bf=self.w1bf_bufs[0], hacc=self.hacc, hconv=self.hconv,
            calt=self.calt, w1bf_alt=self.w1bf_bufs[1] if len(self.w1bf_bufs) > 1 else None, xnext=self.xnext,
            xtag=self.xtag, xcur=self.xcur, ycur=self.ycur, stamps=self.stamps).items() if t is not None}
        ptr.update(eager_w1=int(eager_w1), ppb=ppb)
        if specialised is not None:
            ptr["specialised"] = int(specialised)
        return ptr
