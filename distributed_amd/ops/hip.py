"""Python launchers for the generic-path HIP kernels (csrc/kernels/: gemm.hip and the conv
kernels; bn.hip, pool.hip, loss_head.hip, optimizer.hip, glue.hip, augment.hip).

These are thin, validating wrappers: they check dtypes, shapes, contiguity and the
16-byte alignment the kernels' vector accesses assume, pick the tile shape and split-K
factor, and enqueue on torch's current stream (so everything is captured by a
``torch.cuda.CUDAGraph``).  Activations are NHWC bf16, parameters fp32 masters with
bf16 shadows.  There is no silent fallback: a call that does not meet a kernel's
contract raises.

Keras conventions (reference README.md:58-73): conv kernels ``[kh, kw, cin, cout]``,
dense kernels ``[in, out]``, TF 'same' padding (the extra pixel at bottom/right).
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ..native import require_C

A_KC, A_IM2COL, A_DGRAD, A_MC, A_WGRAD, A_CONV64, A_DGRAD64, A_WGRAD64, A_WGRAD3, A_CONV3, A_DGRAD3 = range(11)
B_NC, B_KC = 0, 1
E_BIAS, E_RELU, E_BF16, E_ATOMIC, E_STATS, E_ADD, E_SLAB, E_BNRED, E_FIXUP = 1, 2, 4, 8, 16, 32, 64, 128, 256
BK = 32


def conv_kstep() -> int:
    """k-step depth of the LDS-DMA conv kernels (csrc/kernels/conv_gemm.hip): 64 (default)
    or 32 (DAMD_CONV_KB=32); the same rule as the C++ side."""
    return 32 if os.environ.get("DAMD_CONV_KB") == "32" else 64


def use_glds(gathered_channels: int) -> bool:
    """The LDS-DMA conv kernels take a conv whose gathered tensor has C % kstep == 0 (one
    filter tap x kstep channels per k-step); DAMD_CONV_GLDS=0 forces the register-staged
    kernel (A/B comparisons)."""
    return gathered_channels % conv_kstep() == 0 and os.environ.get("DAMD_CONV_GLDS", "1") != "0"


def _C():
    return require_C()


def stream_handle() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _chk(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name}: must be a device tensor")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if t.data_ptr() % 16:
        raise ValueError(f"{name}: must be 16-byte aligned")


def same_pad(in_size: int, k: int, s: int) -> Tuple[int, int, int]:
    """TF 'same': (out, pad_before, pad_after)."""
    out = math.ceil(in_size / s)
    total = max((out - 1) * s + k - in_size, 0)
    return out, total // 2, total - total // 2


def conv_out(in_size: int, k: int, s: int, padding: str) -> Tuple[int, int]:
    if padding == "same":
        o, pb, _ = same_pad(in_size, k, s)
        return o, pb
    return (in_size - k) // s + 1, 0


def pick_tile(N: int) -> int:
    """1 -> 256x64 tiles (narrow layers, no wasted MFMA columns), 0 -> 128x128."""
    return 1 if N <= 64 else 0


def tile_rows(tile: int) -> int:
    return 256 if tile == 1 else 128


def tile_count(M: int, N: int, tile: int) -> int:
    """Output tiles (= workgroups per K split) of an [M,N] product."""
    bm, bn = (256, 64) if tile == 1 else (128, 128)
    return -(-M // bm) * -(-N // bn)


def split_k(K: int, tiles: int, target: int, unit: int, limit: int) -> Tuple[int, int]:
    """The split-K rule of every plan below: (splits, k_per_split) of a product summed over K
    whose grid of ``tiles`` workgroups leaves CUs idle.  Enough splits to launch ``target``
    workgroups, at most ``limit`` (the caller's minimum depth per split and slab cap; < 1
    counts as 1); K is cut in multiples of ``unit`` (the kernel's k-step) and splits that
    would be empty after the rounding are dropped."""
    splits = max(1, min(-(-target // tiles), limit))
    kps = -(-(-(-K // unit)) // splits) * unit
    return -(-K // kps), kps


# weight-gradient split-K: every split stores its fp32 partial tile to a slab and one
# reduce kernel adds the slabs into the gradient in fixed order (deterministic; fp32
# atomics from hundreds of blocks on the same addresses serialise at the memory side)
WGRAD_TARGET_WG = int(os.environ.get("DAMD_WGRAD_TARGET_WG", 512))  # 2 workgroups per CU
WGRAD_SLAB_MAX = 64 << 20      # bytes of slab per GEMM


def slab_cap(M: int, N: int) -> int:
    """Most fp32 [M,N] slabs one GEMM may write (WGRAD_SLAB_MAX bytes; at least one)."""
    return max(1, WGRAD_SLAB_MAX // (M * N * 4))


def wgrad_plan(M: int, N: int, K: int) -> Tuple[int, int, int]:
    """(tile, splits, k_per_split) of a weight-gradient GEMM [M,N] summed over K."""
    t = pick_tile(N)
    splits, kps = split_k(K, tile_count(M, N, t), WGRAD_TARGET_WG, BK, min(max(1, K // 256), slab_cap(M, N)))
    return t, splits, kps


# bf16-output GEMMs (conv fwd / dgrad) whose tile count leaves CUs idle are split over K
# into fp32 slabs; splitk_finish then applies the epilogue (bias, residual, ReLU, BN
# statistics per FINISH_RB rows, bf16 store)
SPLIT_MIN_TILES = int(os.environ.get("DAMD_SPLIT_MIN_TILES", 320))
SPLIT_TARGET_WG = int(os.environ.get("DAMD_SPLIT_TARGET_WG", 384))
FINISH_RB = 16


def split_plan(M: int, N: int, K: int, tile: int, bk: int = BK) -> Tuple[int, int]:
    """(splits, k_per_split) for a bf16-output GEMM; splits == 1: the fused epilogue.
    k_per_split is a multiple of the kernel's k-step ``bk``."""
    tiles = tile_count(M, N, tile)
    if tiles >= SPLIT_MIN_TILES:
        return 1, -(-K // bk) * bk
    return split_k(K, tiles, SPLIT_TARGET_WG, bk, min(K // 256, slab_cap(M, N)))


def dense_wgrad_plan(M: int, N: int, K: int) -> dict:
    """Launch plan of the dense weight gradient dw[M,N] summed over K (= batch), in
    conv_wgrad_plan's form: wgrad_plan's tile / splits / kps, the fp32 workspace ``ws`` and
    ``slab1``: an unsplit GEMM over few tiles (the classifier's dW: 32 tiles) stores to one
    slab that the flat reduce adds -- that beats the atomic epilogue there (fp32 atomics
    measured 19 us for the 512 x 1000 dW)."""
    t, splits, kps = wgrad_plan(M, N, K)
    slab1 = splits == 1 and tile_count(M, N, t) <= 64 and (M * N) % 4 == 0 and M * N >= 4 * 8192
    return {"amode": A_MC, "M": M, "N": N, "K": K, "tile": t, "splits": splits, "kps": kps, "kstep": 0,
            "slab1": slab1, "ws": splits * M * N if splits > 1 or slab1 else 0}


def wgrad_workspace_elems(M: int, N: int, K: int) -> int:
    return dense_wgrad_plan(M, N, K)["ws"]


def wgrad64_geo(n: int, ho: int, wo: int, kb: int) -> Tuple[int, int]:
    """(virtual rows, virtual rows per k-step) of the LDS-DMA weight-gradient kernel at
    k-step depth kb (mirror of csrc/kernels/conv_gemm.hip wgrad64_rows / _rows_per_step)."""
    nseg = -(-wo // kb)
    wv = -(-wo // nseg)
    s = 1
    while s < wv:
        s <<= 1
    return n * ho * nseg, kb // s


def wgrad3_ok(n, h, w, cin, cout, k, s, pad) -> bool:
    """Shapes the direct 3x3 weight-gradient kernel takes (mirror of wgrad3_launch)."""
    return (k == 3 and s == 1 and pad == 1 and cin % 64 == 0 and cout % 64 == 0 and w + 1 <= 63
            and n * (h + 1) * (w + 1) + 2048 < (1 << 21))


def conv_wgrad_plan(x_shape, w_shape, strides=(1, 1), padding="valid") -> dict:
    """Launch plan of conv_wgrad.  3x3/stride-1/pad-1 layers with channels % 64 == 0: the
    direct kernel (conv_wgrad3.hip, all nine taps per block).  Otherwise the LDS-DMA
    kernel over virtual rows (conv_gemm.hip) for the packed-tap stem and for layers with
    N = Cout > 64, k-step 32 for images of <= 16 columns (4 blocks/CU: the small-image
    layers are bound by per-block overheads) else 64; the register-staged kernel over
    pixels for N <= 64 (measured faster there: scripts/bench_gemm.py)."""
    n, h, wd, cin, ho, wo, kh, kw, s, pad, cout = conv_geo(x_shape, w_shape, strides, padding)
    M, N = kh * kw * cin, cout
    stem = stem4_ok(x_shape, w_shape, strides, padding)
    pick = os.environ.get("DAMD_WGRAD_KERNEL", "auto")  # auto | direct | glds | reg (tests, A/B runs)
    dma = os.environ.get("DAMD_CONV_GLDS", "1") != "0"
    kstep = 0
    if not stem and dma and pick in ("auto", "direct") and wgrad3_ok(n, h, wd, cin, cout, kh, s, pad):
        # direct 3x3 kernel (csrc/kernels/conv_wgrad3.hip): 64x64 (ci, co) tiles x all 9 taps
        amode, t, K = A_WGRAD3, 0, n * (h + 1) * (wd + 1)
        target = int(os.environ.get("DAMD_WGRAD3_WG", "256"))  # 8-9-wave blocks, 1 per CU
        splits, kps = split_k(K, (cin // 64) * (cout // 64), target, 32,
                              min(max(1, -(-K // 32) // 8), slab_cap(M, N)))
    else:
        kb = int(os.environ.get("DAMD_CONV_KB", "0")) or (32 if wo <= 16 else 64)
        vr, g = wgrad64_geo(n, ho, wo, kb)
        t = pick_tile(N)
        if stem or (dma and (N > 64 if pick == "auto" else pick == "glds") and vr < (1 << 21)):
            if stem:  # packed taps: M = KH x 8 x 4 rows of the stem4_weight_shape layout
                M = kh * 32
            amode, K, kstep = A_WGRAD64, vr, kb
            splits, kps = split_k(K, tile_count(M, N, t), WGRAD_TARGET_WG, g,
                                  min(max(1, -(-K // g) // 4), slab_cap(M, N)))
        else:
            amode, K = A_WGRAD, n * ho * wo
            t, splits, kps = wgrad_plan(M, N, K)
    return {"amode": amode, "M": M, "N": N, "K": K, "tile": t, "splits": splits, "kps": kps, "kstep": kstep,
            "ws": splits * M * N if splits > 1 else 0}


def _wgrad_launch(A, B, dw, ws, plan, *, lda=0, ldb=0, geo=(), accumulate=True, slab1=False, reduce=None):
    """The weight-gradient GEMM dw[M,N] (+)= A^T B of ``plan`` (conv_wgrad_plan /
    dense_wgrad_plan).  One split: the atomic epilogue (one writer per element, an uncontended
    add) unless ``slab1``; otherwise every split stores its fp32 slab to ``ws`` and
    ``reduce(ws)`` (default: the flat splitk_reduce into dw) adds the slabs in fixed order."""
    amode, M, N, K, splits, kstep = (plan[k] for k in ("amode", "M", "N", "K", "splits", "kstep"))
    if splits == 1 and not slab1:
        if not accumulate:
            dw.zero_()
        gemm(A, B, dw, amode=amode, bmode=B_NC, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=N, epi=E_ATOMIC, geo=geo,
             k_per_split=plan["kps"], tile=plan["tile"], kstep=kstep)
        return
    gemm(A, B, ws, amode=amode, bmode=B_NC, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=N, epi=E_SLAB,
         splits=splits, k_per_split=plan["kps"], tile=plan["tile"], geo=geo, kstep=kstep)
    if reduce is not None:
        reduce(ws)
    else:
        _C().splitk_reduce(_ptr(ws), splits, M * N, _ptr(dw), stream_handle(), accumulate=int(accumulate))


def acc_reps(acc, C: int, words: int) -> int:
    """Replica count of a BatchNorm statistics accumulator of C channels (int64 fixed point,
    layer_ops.h BNFin / BNBwdFin), after checking its layout: ``words`` per channel (2 forward,
    4 backward) in [reps + 1, words C] (2-D: the last row is the sticky non-finite flag plane,
    damd_common.h bnacc_flag) or one replica + its flag plane (1-D, [2 words C]).  Producer
    block b adds into replica b % reps, and every kernel writes the flag plane behind the last
    replica: a tensor without it would be written past its end, so this raises instead."""
    if acc.dtype != torch.int64 or not acc.is_contiguous():
        raise ValueError("a BatchNorm accumulator is a contiguous int64 tensor")
    K = words * C
    if acc.dim() == 2 and acc.shape[0] >= 2 and acc.shape[1] == K:
        return int(acc.shape[0]) - 1
    if acc.dim() == 1 and acc.numel() == 2 * K:
        return 1
    raise ValueError(f"a BatchNorm accumulator is [reps + 1, {K}] (replicas + the flag row) or [{2 * K}], "
                     f"got {tuple(acc.shape)}")


def acc_zeros(reps: int, K: int, device) -> torch.Tensor:
    """A cleared accumulator of ``reps`` replicas of K words + the flag plane."""
    return torch.zeros(reps + 1, K, dtype=torch.int64, device=device)


# Fixed-point BatchNorm accumulators (csrc/include/damd_common.h bnacc_add1 / bnacc_add2):
# integer atomics, so the statistics are bitwise independent of the producer blocks'
# arrival order.  Forward sums: one int64 word per value (unit 2^-24); backward sums: two
# (hi = floor(v 2^24), lo = floor((v 2^24 - hi) 2^40)) in planes [s hi | s lo | q hi | q lo].
ACC_UNIT = 2.0 ** -24


def bn_acc_encode(values: torch.Tensor, words: int = 1) -> torch.Tensor:
    """Host encoding of fp64 sums into accumulator words (tests / diagnostics): [..., 2C]
    doubles (sums, second statistics) -> [..., 2C] (words 1) or [..., 4C] (words 2: planes
    s hi | s lo | q hi | q lo) int64."""
    v = values.double().cpu()
    if words == 1:
        return torch.round(v * 2.0 ** 24).to(torch.int64)
    d = v * 2.0 ** 24
    hi = torch.floor(d)
    lo = torch.floor((d - hi) * 2.0 ** 40)
    C = v.shape[-1] // 2
    parts = [hi[..., :C], lo[..., :C], hi[..., C:], lo[..., C:]]
    return torch.cat([p.to(torch.int64) for p in parts], -1)


def bn_acc_decode(acc: torch.Tensor, words: int = 1) -> torch.Tensor:
    """Replica-summed values of an accumulator ([reps + 1, K] or [2K]: replicas then the flag
    plane) as fp64; NaN where a channel's flag is set."""
    a = acc.cpu()
    if a.dim() == 1:
        a = a.view(2, -1)
    flag = a[-1]
    a = a[:-1].sum(0)
    if words == 1:
        C = a.numel() // 2
        out = a.double() * ACC_UNIT
        bad = torch.cat([flag[:C] != 0] * 2)
    else:
        C = a.numel() // 4
        s = a[:C].double() * ACC_UNIT + a[C:2 * C].double() * 2.0 ** -64
        q = a[2 * C:3 * C].double() * ACC_UNIT + a[3 * C:].double() * 2.0 ** -64
        out = torch.cat([s, q])
        bad = torch.cat([flag[:C] != 0] * 2)
    out[bad] = float("nan")
    return out


def _stats_ptrs(stats, N, words=2):
    """(partials pointer, accumulator pointer, replicas) of a stats argument over N columns:
    an fp32 [T][2][N] partials tensor, or an int64 fixed-point accumulator (acc_reps) of 2
    words per column (forward) or 4 (backward, E_BNRED) (BNFin: producers add, the consumer
    finalizes)."""
    if stats is None:
        return 0, 0, 1
    if stats.dtype == torch.int64:
        return 0, _ptr(stats), acc_reps(stats, N, words)
    return _ptr(stats), 0, 1


def gemm(A, B, C, *, amode, bmode, M, N, K, lda=0, ldb=0, ldc=0, epi=0, bias=None, stats=None, R=None,
         geo: Sequence[int] = (), kc=0, splits=1, k_per_split=None, tile=None, kstep=0, bnx=None, bnst=None,
         bnin=None, slab=None):
    t = pick_tile(N) if tile is None else tile
    kps = k_per_split if k_per_split is not None else -(-K // BK) * BK
    sp, sa, reps = _stats_ptrs(stats, N, 4 if epi & E_BNRED else 2)
    bp, bv = bnin[0].args() if bnin is not None else ([], [])
    _C().gemm(amode, bmode, epi, splits, t, _ptr(A), _ptr(B), _ptr(C), _ptr(bias), sp, _ptr(R), M, N, K,
              lda, ldb, ldc, list(geo), kc, kps, stream_handle(), kstep, stats_acc=sa, bnx=_ptr(bnx), bnst=_ptr(bnst),
              stats_reps=reps, bnin_p=bp, bnin_v=bv, bnin_y=_ptr(bnin[1]) if bnin is not None else 0,
              slab=_ptr(slab), tickets=_ptr(_tickets(A.device)) if epi & E_FIXUP else 0)


_TICKETS = {}


def _tickets(device) -> torch.Tensor:
    """The per-tile arrival tickets of the in-launch split-K finish (E_FIXUP): zero between
    launches (each tile's reducing split resets its own), shared by the launches of one
    stream in order."""
    t = _TICKETS.get(device)
    if t is None:
        t = _TICKETS[device] = torch.zeros(1 << 16, dtype=torch.int32, device=device)
    return t


def splitk_fixup_on(stats) -> bool:
    """Split-K GEMMs finish inside the launch (E_FIXUP) with DAMD_SPLITK_FIXUP=1 when the BN
    statistics (if any) go to a fixed-point accumulator.  Off by default: measured on the
    ResNet-18 step, 2.704 vs 2.587 ms -- the last split of a 128 x 128 tile re-reads S x 64 KB
    of slabs serially (layer-4 forward 26 -> 48 us per conv against the 8 us finish launch
    it replaces); the in-launch reduction pays only for slabs of a few tens of KB per tile."""
    return os.environ.get("DAMD_SPLITK_FIXUP", "0") == "1" and (stats is None or stats.dtype == torch.int64)


# ---- dense -------------------------------------------------------------------------------
# Small-M dense GEMMs (a 64-row batch against a 512 x 1000 classifier) give 4-8 output
# tiles: 4-8 busy CUs walking 8-16 serial k-steps (23-32 us on MI355X for <= 66 MFLOP).
# They are split over K into fp32 slabs (one k-step or two per workgroup) and finished by
# a fixed-order reduction kernel with the bias / ReLU / accumulate epilogue.
DENSE_SPLIT_MAX_TILES = 32
DENSE_SPLIT_TARGET_WG = int(os.environ.get("DAMD_DENSE_SPLIT_WG", "128"))  # 1: no split-K (A/B runs)


def dense_split_plan(M: int, N: int, K: int) -> Tuple[int, int]:
    """(splits, k_per_split) of a dense forward / backprop-input GEMM [M,N] over K."""
    tiles = tile_count(M, N, pick_tile(N))
    if tiles > DENSE_SPLIT_MAX_TILES or K < 2 * BK:
        return 1, -(-K // BK) * BK
    return split_k(K, tiles, DENSE_SPLIT_TARGET_WG, BK, K // BK)


def dense_workspace_elems(M: int, N: int, K: int) -> int:
    """fp32 workspace of the split forward (x[M,K] @ w[K,N]) and backprop-input GEMMs."""
    s1, _ = dense_split_plan(M, N, K)
    s2, _ = dense_split_plan(M, K, N)
    return max(s1 * M * N if s1 > 1 else 0, s2 * M * K if s2 > 1 else 0)


def dense_fwd(x: torch.Tensor, w: torch.Tensor, out: torch.Tensor, bias=None, relu=False, stats=None,
              workspace: Optional[torch.Tensor] = None):
    """out[M,N] = x[M,K] @ w[K,N] (+bias)(relu); x, w bf16; out bf16 or fp32.  With a
    workspace, under-filled shapes run split-K (dense_split_plan)."""
    M, K = x.shape
    K2, N = w.shape
    assert K == K2 and tuple(out.shape) == (M, N)
    _chk(x, torch.bfloat16, "x")
    _chk(w, torch.bfloat16, "w")
    if K % 8 or N % 8:
        raise ValueError("dense_fwd: K and N must be multiples of 8 (pad the layer)")
    splits, kps = dense_split_plan(M, N, K)
    if splits > 1 and stats is None and workspace is not None and workspace.numel() >= splits * M * N:
        gemm(x, w, workspace, amode=A_KC, bmode=B_NC, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, epi=E_SLAB,
             splits=splits, k_per_split=kps)
        if out.dtype == torch.float32:
            _C().splitk_finish_f32(_ptr(workspace), splits, M, N, _ptr(bias), int(relu), _ptr(out), N,
                                   stream_handle())
        else:
            _C().splitk_finish(_ptr(workspace), splits, M, N, _ptr(bias), 0, int(relu), 0, FINISH_RB, _ptr(out), N,
                               stream_handle())
        return
    epi = (E_BIAS if bias is not None else 0) | (E_RELU if relu else 0)
    epi |= E_BF16 if out.dtype == torch.bfloat16 else 0
    if stats is not None:
        epi |= E_STATS
    gemm(x, w, out, amode=A_KC, bmode=B_NC, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, epi=epi, bias=bias, stats=stats)


def dense_dgrad(dy: torch.Tensor, w: torch.Tensor, dx: torch.Tensor, accumulate=False,
                workspace: Optional[torch.Tensor] = None):
    """dx[M,K] (+)= dy[M,N] @ w[K,N]^T (bf16 out); split-K with a workspace like dense_fwd."""
    M, N = dy.shape
    K, N2 = w.shape
    assert N == N2 and tuple(dx.shape) == (M, K)
    _chk(dy, torch.bfloat16, "dy")
    _chk(w, torch.bfloat16, "w")
    _chk(dx, torch.bfloat16, "dx")
    splits, kps = dense_split_plan(M, K, N)
    if splits > 1 and workspace is not None and workspace.numel() >= splits * M * K:
        gemm(dy, w, workspace, amode=A_KC, bmode=B_KC, M=M, N=K, K=N, lda=N, ldc=K, epi=E_SLAB, kc=N,
             splits=splits, k_per_split=kps)
        _C().splitk_finish(_ptr(workspace), splits, M, K, 0, _ptr(dx) if accumulate else 0, 0, 0, FINISH_RB,
                           _ptr(dx), K, stream_handle())
        return
    epi = E_BF16 | (E_ADD if accumulate else 0)
    gemm(dy, w, dx, amode=A_KC, bmode=B_KC, M=M, N=K, K=N, lda=N, ldc=K, epi=epi, kc=N,
         R=dx if accumulate else None)


def dense_wgrad(x: torch.Tensor, dy: torch.Tensor, dw: torch.Tensor, workspace: Optional[torch.Tensor] = None,
                accumulate: bool = True):
    """dw[K,N] (+)= x[M,K]^T @ dy[M,N] (fp32; split over M, slabs reduced in fixed order);
    accumulate=False overwrites dw."""
    M, K = x.shape
    M2, N = dy.shape
    assert M == M2 and tuple(dw.shape) == (K, N)
    _chk(x, torch.bfloat16, "x")
    _chk(dy, torch.bfloat16, "dy")
    _chk(dw, torch.float32, "dw")
    plan = dense_wgrad_plan(K, N, M)
    if workspace is None and plan["ws"]:
        workspace = torch.empty(plan["ws"], device=x.device)
    # (a caller's workspace too small for the one-slab route: the atomic epilogue instead)
    slab1 = plan["slab1"] and workspace.numel() >= K * N
    need = plan["splits"] * K * N
    if (plan["splits"] > 1 or slab1) and (workspace.numel() < need or workspace.dtype != torch.float32):
        raise ValueError(f"weight-gradient GEMM needs an fp32 workspace of {need} elements")
    _wgrad_launch(x, dy, dw, workspace, plan, lda=K, ldb=N, accumulate=accumulate, slab1=slab1)


# ---- conv ---------------------------------------------------------------------------------
def conv_geo(x_shape, w_shape, strides, padding):
    n, h, w_, c = x_shape
    kh, kw, cin, cout = w_shape
    if strides[0] != strides[1] or kh != kw or h != w_:
        raise ValueError("HIP conv path: square kernels/images and equal strides only")
    ho, pad = conv_out(h, kh, strides[0], padding)
    wo, pad2 = conv_out(w_, kw, strides[1], padding)
    assert pad == pad2
    return n, h, w_, cin, ho, wo, kh, kw, strides[0], pad, cout


def stem4_ok(x_shape, w_shape, strides, padding) -> bool:
    """A conv the packed-tap stem kernels take (conv_gemm.hip): a 4-channel input (e.g.
    RGB + one zero channel), a square kernel of <= 8 columns, even stride, even top/left
    padding and an even image width.  Its weights are laid out [KH][8][4][Cout] (zero
    beyond the true KW columns / Cin channels): stem4_weight_layout."""
    n, h, wd, cin, ho, wo, kh, kw, s, pad, cout = conv_geo(x_shape, w_shape, strides, padding)
    return (cin == 4 and kw <= 8 and s % 2 == 0 and pad % 2 == 0 and wd % 2 == 0 and cout % 8 == 0
            and os.environ.get("DAMD_CONV_GLDS", "1") != "0")


def stem4_weight_shape(w_shape):
    kh, kw, cin, cout = w_shape
    return (kh, 8, 4, cout)


def conv_fwd_stem4(x, w8, out, kernel_size, strides=(2, 2), padding="same", bias=None, relu=False, stats=None,
                   workspace: Optional[torch.Tensor] = None):
    """Packed-tap stem forward: out = conv(x [N,H,W,4], true kernel kernel_size x
    kernel_size) with w8 = the weights in stem4_weight_shape layout (bf16)."""
    k = kernel_size
    cout = w8.shape[-1]
    wshape = (k, k, 4, cout)
    if not stem4_ok(x.shape, wshape, strides, padding) or tuple(w8.shape) != stem4_weight_shape(wshape):
        raise ValueError("conv_fwd_stem4: not a packed-tap stem conv")
    _chk(x, torch.bfloat16, "x")
    _chk(w8, torch.bfloat16, "w8")
    n, h, wd, cin, ho, wo, kh, kw, s, pad, cout = conv_geo(x.shape, wshape, strides, padding)
    assert tuple(out.shape) == (n, ho, wo, cout)
    plan = conv_fwd_plan(x.shape, wshape, strides, padding)
    _check_stats(stats, plan, cout, "conv_fwd_stem4")
    _conv_fwd_launch(x, w8, out, plan, (h, wd, 4, ho, wo, kh, 8, s, pad), bias, relu, stats, workspace, kstep=32)


def _check_stats(stats, plan, cout, who):
    if stats is None:
        return
    if stats.dtype == torch.int64:
        acc_reps(stats, cout, 2)
    elif stats.shape[0] != plan["stats_T"]:
        raise ValueError(f"{who}: stats needs {plan['stats_T']} partial rows, got {stats.shape[0]}")


def conv_wgrad_stem4(x, dy, dw8, kernel_size, strides=(2, 2), padding="same",
                     workspace: Optional[torch.Tensor] = None, accumulate: bool = True,
                     dw: Optional[torch.Tensor] = None) -> bool:
    """Packed-tap stem weight gradient: dw8 [KH][8][4][Cout] (fp32) += the gradient in the
    stem4_weight_shape layout (entries beyond the true kernel are junk to drop).  With
    ``dw`` (the true [KH][KW][Cin][Cout] fp32 gradient) and a split-K plan, the split-K
    reduce drops the junk and ADDS straight into ``dw`` (dw8 untouched; ``accumulate``
    applies to dw8 only); returns True then, else False (the caller unpads dw8 itself)."""
    k = kernel_size
    cout = dw8.shape[-1]
    wshape = (k, k, 4, cout)
    if not stem4_ok(x.shape, wshape, strides, padding) or tuple(dw8.shape) != stem4_weight_shape(wshape):
        raise ValueError("conv_wgrad_stem4: not a packed-tap stem conv")
    _chk(x, torch.bfloat16, "x")
    _chk(dy, torch.bfloat16, "dy")
    _chk(dw8, torch.float32, "dw8")
    plan = conv_wgrad_plan(x.shape, wshape, strides, padding)
    n, h, wd, cin, ho, wo, kh, kw, s, pad, cout = conv_geo(x.shape, wshape, strides, padding)
    geo = (h, wd, 4, ho, wo, kh, 8, s, pad)
    splits = plan["splits"]

    def reduce_unpad(ws):  # the reduce's rows [KH][8][4 x Cout] -> [KH][KW][Cin x Cout]
        _chk(dw, torch.float32, "dw")
        ci = dw.shape[2] if dw.dim() == 4 else 0
        if tuple(dw.shape) != (k, k, ci, cout) or not 1 <= ci <= 4:
            raise ValueError(f"conv_wgrad_stem4: dw shape {tuple(dw.shape)} is not [{k}][{k}][<=4][{cout}]")
        _C().splitk_reduce_unpad(_ptr(ws), splits, k, k, ci * cout, 8, 4 * cout, _ptr(dw), stream_handle(), 1)

    unpad = dw is not None and splits > 1
    _wgrad_launch(x, dy, dw8, _workspace(workspace, plan["ws"], x.device), plan, ldb=cout, geo=geo,
                  accumulate=accumulate, reduce=reduce_unpad if unpad else None)
    return unpad


# ---- direct 3x3 / stride-1 / pad-1 convolution (csrc/kernels/conv3x3.hip) ---------------


def conv3_rows(h: int, w: int, bn: int) -> int:
    """Output rows per block of the direct 3x3 kernel (mirror of conv3x3.hip conv3_rows):
    the block's R x W pixels fill its 256 (BN 64) / 128 (BN 128) MFMA rows and the input
    halo + weight ring fit 80 KiB (two blocks per CU); 0 = shape not taken."""
    bm = 256 if bn == 64 else 128
    r = min(bm // w, h)
    if r < 1:
        return 0
    halo = (((r + 2) * (w + 2)) * 128 + 1023) & ~1023
    return r if halo + (4 if bn == 64 else 3) * bn * 128 <= 80 * 1024 else 0


def conv3_tile(n: int, h: int, w: int, gathered: int, out_ch: int):
    """(tile, rows, row blocks per image) when the direct kernel takes a 3x3/s1/p1 conv of
    ``gathered`` input channels into ``out_ch`` on n x h x w images, else None: channels %
    64, the block's pixels fill >= 3/4 of its MFMA rows, and the grid has >= CONV3_MIN_WG
    blocks (DAMD_CONV3_MIN_WG, default 256: ResNet layers 1-3; smaller grids keep the split-K implicit GEMM)."""
    if os.environ.get("DAMD_CONV3", "1") == "0" or os.environ.get("DAMD_CONV_GLDS", "1") == "0":
        return None
    if gathered % 64 or out_ch % 64:
        return None
    bn = 64 if out_ch % 128 else 128
    r = conv3_rows(h, w, bn)
    if r == 0 or r * w < 0.75 * (256 if bn == 64 else 128):
        return None
    tpi = -(-h // r)
    if (out_ch // bn) * n * tpi < int(os.environ.get("DAMD_CONV3_MIN_WG", 256)):
        return None
    return (1 if bn == 64 else 0), r, tpi


def conv_fwd_plan(x_shape, w_shape, strides=(1, 1), padding="valid") -> dict:
    """Launch plan of conv_fwd: tile, split-K, number of BN-statistics partials and the
    fp32 workspace it needs (0 when not split)."""
    n, h, wd, cin, ho, wo, kh, kw, s, pad, cout = conv_geo(x_shape, w_shape, strides, padding)
    if stem4_ok(x_shape, w_shape, strides, padding):
        # packed-tap stem: K = KH x (8 pixels x 4 channels), k-step 32 (conv_gemm.hip)
        M, N, K = n * ho * wo, cout, kh * 32
        t = pick_tile(N)
        splits, kps = split_plan(M, N, K, t, 32)
        return {"M": M, "N": N, "K": K, "tile": t, "splits": splits, "kps": kps, "amode": A_CONV64,
                "kstep": 32, "stats_T": -(-M // (FINISH_RB if splits > 1 else tile_rows(t))),
                "ws": splits * M * N if splits > 1 else 0}
    M, N, K = n * ho * wo, cout, kh * kw * cin
    c3 = conv3_tile(n, h, wd, cin, cout) if (kh == kw == 3 and s == 1 and pad == 1 and ho == h) else None
    if c3 is not None:
        return {"M": M, "N": N, "K": K, "tile": c3[0], "splits": 1, "kps": K, "amode": A_CONV3,
                "stats_T": n * c3[2], "ws": 0}
    t = pick_tile(N)
    glds = use_glds(cin)
    splits, kps = split_plan(M, N, K, t, conv_kstep() if glds else BK)
    return {"M": M, "N": N, "K": K, "tile": t, "splits": splits, "kps": kps,
            "amode": A_CONV64 if glds else A_IM2COL,
            "stats_T": -(-M // (FINISH_RB if splits > 1 else tile_rows(t))),
            "ws": splits * M * N if splits > 1 else 0}


def conv_fwd(x, w, out, strides=(1, 1), padding="valid", bias=None, relu=False, stats=None,
             workspace: Optional[torch.Tensor] = None, bnin=None):
    """out [N,Ho,Wo,Cout] = conv(x [N,H,W,Cin], w [KH,KW,Cin,Cout]); bf16 in/out.  stats
    (BN batch statistics partials) must have conv_fwd_plan(...)["stats_T"] rows.
    bnin = (fin: BNFin, y): x is a BatchNorm's input and the conv runs on y = relu(BN(x)),
    finalized and applied on load by the direct kernel (A_CONV3 plans only), which also
    stores y (bitwise bn_apply(x, fin, y, relu=True)) and publishes fin's st / moving
    statistics."""
    n, h, wd, cin, ho, wo, kh, kw, s, pad, cout = conv_geo(x.shape, w.shape, strides, padding)
    _chk(x, torch.bfloat16, "x")
    _chk(w, torch.bfloat16, "w")
    if cin % 8 or cout % 8:
        raise ValueError("conv_fwd: Cin and Cout must be multiples of 8 (pad the channels)")
    assert tuple(out.shape) == (n, ho, wo, cout)
    plan = conv_fwd_plan(x.shape, w.shape, strides, padding)
    _check_stats(stats, plan, cout, "conv_fwd")
    geo = (h, wd, cin, ho, wo, kh, kw, s, pad)
    if bnin is not None and (plan["amode"] != A_CONV3 or plan["splits"] != 1 or bnin[0].acc is None
                             or tuple(bnin[1].shape) != tuple(x.shape)):
        raise ValueError("conv_fwd: a BN input needs a direct 3x3 plan and y of x's shape")
    _conv_fwd_launch(x, w, out, plan, geo, bias, relu, stats, workspace, bnin=bnin, fixup=True)


def _conv_fwd_launch(x, w, out, plan, geo, bias, relu, stats, workspace, *, kstep=0, bnin=None, fixup=False):
    """The forward GEMM of ``plan``: the fused epilogue for one split, else fp32 slabs +
    splitk_finish (``fixup``: finished inside the launch where splitk_fixup_on allows)."""
    M, K, cout = plan["M"], plan["K"], plan["N"]
    epi = (E_BIAS if bias is not None else 0) | (E_RELU if relu else 0) | E_BF16 | (E_STATS if stats is not None else 0)
    if plan["splits"] == 1:
        gemm(x, w, out, amode=plan["amode"], bmode=B_NC, M=M, N=cout, K=K, ldb=cout, ldc=cout, epi=epi,
             bias=bias, stats=stats, geo=geo, tile=plan["tile"], kstep=kstep, bnin=bnin)
        return
    ws = _workspace(workspace, plan["ws"], x.device)
    if fixup and plan["amode"] == A_CONV64 and splitk_fixup_on(stats) and cout % 4 == 0 \
            and not (relu and stats is not None):  # (no kernel instantiates both)
        gemm(x, w, out, amode=plan["amode"], bmode=B_NC, M=M, N=cout, K=K, ldb=cout, ldc=cout, epi=E_FIXUP | epi,
             bias=bias, stats=stats, splits=plan["splits"], k_per_split=plan["kps"], tile=plan["tile"], geo=geo,
             slab=ws)
        return
    gemm(x, w, ws, amode=plan["amode"], bmode=B_NC, M=M, N=cout, K=K, ldb=cout, ldc=cout, epi=E_SLAB,
         splits=plan["splits"], k_per_split=plan["kps"], tile=plan["tile"], geo=geo, kstep=kstep)
    sp, sa, reps = _stats_ptrs(stats, cout)
    _C().splitk_finish(_ptr(ws), plan["splits"], M, cout, _ptr(bias), 0, int(relu), sp, FINISH_RB,
                       _ptr(out), cout, stream_handle(), stats_acc=sa, stats_reps=reps)


def _workspace(ws, need, device):
    if need == 0:
        return None
    if ws is None:
        return torch.empty(need, device=device)
    if ws.dtype != torch.float32 or ws.numel() < need:
        raise ValueError(f"split-K GEMM needs an fp32 workspace of {need} elements")
    return ws


def conv_dgrad_plan(dx_shape, w_shape, strides=(1, 1), padding="valid") -> dict:
    n, h, wd, cin, ho, wo, kh, kw, s, pad, cout = conv_geo(dx_shape, w_shape, strides, padding)
    M, N, K = n * h * wd, cin, kh * kw * cout
    c3 = conv3_tile(n, h, wd, cout, cin) if (kh == kw == 3 and s == 1 and pad == 1 and ho == h) else None
    if c3 is not None:
        return {"M": M, "N": N, "K": K, "tile": c3[0], "splits": 1, "kps": K, "amode": A_DGRAD3, "ws": 0,
                "stats_T": n * c3[2]}
    t = pick_tile(N)
    if (s == 2 and use_glds(cout) and h % 2 == 0 and wd % 2 == 0 and pad == 0
            and os.environ.get("DAMD_DGRAD_SUBPIX", "1") != "0"):
        # stride 2: four sub-pixel classes (conv_gemm.hip), rows = one class grid, no K split
        return {"M": n * (h // 2) * (wd // 2), "N": N, "K": K, "tile": t, "splits": 1, "kps": K,
                "amode": A_DGRAD64, "ws": 0}
    glds = s == 1 and use_glds(cout)
    splits, kps = split_plan(M, N, K, t, conv_kstep() if glds else BK)
    return {"M": M, "N": N, "K": K, "tile": t, "splits": splits, "kps": kps,
            "amode": A_DGRAD64 if glds else A_DGRAD,
            "ws": splits * M * N if splits > 1 else 0}


def conv_dgrad(dy, w, dx, strides=(1, 1), padding="valid", accumulate=False,
               workspace: Optional[torch.Tensor] = None, bnred=None) -> bool:
    """dx [N,H,W,Cin] (+)= backprop-input of dy [N,Ho,Wo,Cout] through w.  ``bnred`` =
    (x, st, part): dx is the gradient of relu(BN(x)) (BN coefficients st [4][Cin]); when the
    direct kernel runs (conv_dgrad_plan stats_T rows) it also writes the BN-backward
    partials (sum dz, sum dz * xhat per tile) into part [stats_T][2][Cin] (or adds them into
    an int64 fixed-point accumulator [reps + 1][4 Cin]: two words per value, then the flag
    row; acc_reps), replacing bn_bwd_reduce.  Returns True when it did."""
    n, h, wd, cin, ho, wo, kh, kw, s, pad, cout = conv_geo(dx.shape, w.shape, strides, padding)
    if s not in (1, 2):
        raise ValueError("conv_dgrad: stride 1 or 2")
    _chk(dy, torch.bfloat16, "dy")
    _chk(w, torch.bfloat16, "w")
    _chk(dx, torch.bfloat16, "dx")
    if cin % 8 or cout % 8:
        raise ValueError("conv_dgrad: Cin and Cout must be multiples of 8")
    plan = conv_dgrad_plan(dx.shape, w.shape, strides, padding)
    M, K = plan["M"], plan["K"]
    geo = (h, wd, cout, ho, wo, kh, kw, s, pad)
    if bnred is not None and plan["amode"] == A_DGRAD3 and not accumulate:
        bx, bst, part = bnred
        if part.dtype == torch.int64:  # a fixed-point accumulator (BNBwdFin)
            acc_reps(part, cin, 4)
        elif part.shape[0] != plan["stats_T"]:
            raise ValueError("conv_dgrad: bnred partials do not match the plan")
        if tuple(bx.shape) != tuple(dx.shape):
            raise ValueError("conv_dgrad: bnred BN input does not match dx")
        gemm(dy, w, dx, amode=A_DGRAD3, bmode=B_KC, M=M, N=cin, K=K, ldc=cin, epi=E_BF16 | E_BNRED, kc=cout,
             geo=geo, stats=part, tile=plan["tile"], bnx=bx, bnst=bst)
        return True
    if plan["splits"] == 1:
        epi = E_BF16 | (E_ADD if accumulate else 0)
        gemm(dy, w, dx, amode=plan["amode"], bmode=B_KC, M=M, N=cin, K=K, ldc=cin, epi=epi, kc=cout, geo=geo,
             R=dx if accumulate else None, tile=plan["tile"])
        return False
    ws = _workspace(workspace, plan["ws"], dx.device)
    if plan["amode"] == A_DGRAD64 and splitk_fixup_on(None) and cin % 4 == 0:
        gemm(dy, w, dx, amode=plan["amode"], bmode=B_KC, M=M, N=cin, K=K, ldc=cin,
             epi=E_FIXUP | E_BF16 | (E_ADD if accumulate else 0), kc=cout, geo=geo, R=dx if accumulate else None,
             splits=plan["splits"], k_per_split=plan["kps"], tile=plan["tile"], slab=ws)
        return False
    gemm(dy, w, ws, amode=plan["amode"], bmode=B_KC, M=M, N=cin, K=K, ldc=cin, epi=E_SLAB, kc=cout, geo=geo,
         splits=plan["splits"], k_per_split=plan["kps"], tile=plan["tile"])
    _C().splitk_finish(_ptr(ws), plan["splits"], M, cin, 0, _ptr(dx) if accumulate else 0, 0, 0, FINISH_RB,
                       _ptr(dx), cin, stream_handle())
    return False


def conv_wgrad_workspace_elems(x_shape, w_shape, strides=(1, 1), padding="valid") -> int:
    return conv_wgrad_plan(x_shape, w_shape, strides, padding)["ws"]


def conv_wgrad(x, dy, dw, strides=(1, 1), padding="valid", workspace: Optional[torch.Tensor] = None,
               accumulate: bool = True):
    """dw [KH,KW,Cin,Cout] (+)= sum over pixels of im2col(x)^T dy (split-K over pixels, fp32
    slabs in ``workspace`` (conv_wgrad_workspace_elems) reduced in fixed order);
    accumulate=False overwrites dw (no zeroing pass)."""
    n, h, wd, cin, ho, wo, kh, kw, s, pad, cout = conv_geo(x.shape, dw.shape, strides, padding)
    _chk(x, torch.bfloat16, "x")
    _chk(dy, torch.bfloat16, "dy")
    _chk(dw, torch.float32, "dw")
    if cin % 8 or cout % 8:
        raise ValueError("conv_wgrad: Cin and Cout must be multiples of 8")
    plan = conv_wgrad_plan(x.shape, dw.shape, strides, padding)
    _wgrad_launch(x, dy, dw, _workspace(workspace, plan["ws"], x.device), plan, ldb=cout,
                  geo=(h, wd, cin, ho, wo, kh, kw, s, pad), accumulate=accumulate)


# ---- BatchNorm / pooling ------------------------------------------------------------------------
# One launcher per op, two carriers of the batch statistics.  The caller names the carrier; it
# is never guessed from a dtype.
# * partials: producers (a GEMM epilogue with fp32 `stats`, bn_stats, bn_bwd_reduce) write fp32
#   per-block rows part [T][2][C]; bn_finalize / bn_bwd_finalize launches turn them into st / co.
#   Forward argument: the st tensor; backward: part.
# * accumulators: producers (the same epilogues with an int64 `stats`, the split-K finish,
#   bn_bwd_reduce) add into int64 fixed point ([reps + 1, 2C] forward, [reps + 1, 4C] backward,
#   acc_reps: block b into replica b % reps; integer sums, so independent of the blocks' arrival
#   order) and the consumer finalizes in its prologue (layer_ops.h BNFin / BNBwdFin): no finalize
#   launch.  Forward argument: a BNFin in place of st; backward: acc.  The accumulators must be
#   zero before the producers run (the native graph engine clears them in gather_batch).
FIN_MAX_C = 4096
STEM_FUSE_MAX_C = 2048  # pool.hip pool_bn_bwd_reduce: C / 8 channel groups within one 256-thread block


class BNFin:
    """Forward finalize parameters of one BatchNorm: int64 accumulator acc [reps + 1][2 C]
    (per replica the sums, then the sums of squares of the BN input; the last row is the flag
    plane; acc_reps) or None (the consumer reads st), gamma / beta (None: 1 / 0), st [4][C]
    written by the consumer's block 0 (mean, invstd, scale, shift), moving statistics (None:
    not updated), the element count per channel, epsilon and the moving-average momentum."""

    def __init__(self, acc, gamma, beta, st, rmean, rvar, count, eps, momentum):
        self.acc, self.st = acc, st
        if acc is None:
            reps = 1
        elif st is None:
            raise ValueError("BNFin: an accumulator needs st [4][C] to finalize into")
        else:
            reps = acc_reps(acc, st.numel() // 4, 2)
        self._p = [_ptr(acc), _ptr(gamma), _ptr(beta), _ptr(st), _ptr(rmean), _ptr(rvar)]
        self._v = [float(count), float(eps), float(momentum), float(reps)]

    def args(self):
        return self._p, self._v


def _fwd_stats(st):
    """(st pointer, BNFin pointers, BNFin values) of a forward statistics argument."""
    return (_ptr(st.st), *st.args()) if isinstance(st, BNFin) else (_ptr(st), [], [])


def _bwd_stats(part, acc, M, C, co, dgamma, dbeta, who):
    """(reduce keywords, apply keywords) of a backward carrier: none for partials, the checked
    accumulator (acc_reps) and what its apply finalizes into for acc."""
    if (part is None) == (acc is None):
        raise ValueError(f"{who}: exactly one of part (fp32 partials) and acc (int64 accumulator)")
    if acc is None:
        return {}, {}
    reps = acc_reps(acc, C, 4)
    return (dict(acc=_ptr(acc), reps=reps),
            dict(bfin=[_ptr(acc), _ptr(dgamma), _ptr(dbeta), _ptr(co)], count=float(M), reps=reps))


def bn_bwd_blocks(M: int, C: int) -> int:
    return _C().bn_bwd_blocks(M, C)


def bn_stats(x, ident, part):
    """Sum and sum of squares of x [.., C] per channel into the fp32 partials part [T][2][C]
    (bn_bwd_reduce against ident = rows (0, 1, 1, 0): mean 0, invstd 1); returns T.  Partials
    only: the kernel adds into an accumulator in the backward two-word layout, which no forward
    consumer (BNFin: one word per value) decodes."""
    if part.dtype != torch.float32:
        raise ValueError("bn_stats: fp32 partials (the kernel cannot write a forward accumulator)")
    C = x.shape[-1]
    M = x.numel() // C
    T = bn_bwd_blocks(M, C)
    assert part.numel() >= T * 2 * C
    _C().bn_bwd_reduce(_ptr(x), 0, 0, _ptr(x), _ptr(ident), 0, _ptr(part), T, M, C, stream_handle())
    return T


def bn_finalize(part, T, C, count, gamma, beta, eps, momentum, rmean, rvar, st):
    _C().bn_finalize(_ptr(part), T, C, float(count), _ptr(gamma), _ptr(beta), float(eps), float(momentum),
                     _ptr(rmean), _ptr(rvar), _ptr(st), stream_handle())


def bn_infer_st(rmean, rvar, gamma, beta, eps, st):
    """st [4][C] of the moving statistics (inference): what bn_finalize leaves for a batch."""
    _C().bn_infer_st(_ptr(rmean), _ptr(rvar), _ptr(gamma), _ptr(beta), float(eps), st.shape[-1], _ptr(st),
                     stream_handle())


def bn_apply(x, st, y, relu=False, r=None, st2=None):
    """y = act(BN(x) [+ r | + BN2(r)]); st / st2: each an fp32 [4][C] tensor or a BNFin."""
    C = x.shape[-1]
    M = x.numel() // C
    mode = 0 if r is None else (1 if st2 is None else 2)
    s1, p1, v1 = _fwd_stats(st)
    s2, p2, v2 = _fwd_stats(st2)
    _C().bn_apply(_ptr(x), s1, _ptr(r), s2, mode, int(relu), _ptr(y), M, C, stream_handle(), fin=p1, fin_v=v1,
                  fin2=p2, fin2_v=v2)


def bn_bwd(dy, y, relu_mask, x, st, part, co, dx, dgamma=None, dbeta=None, dz_out=None, acc=None, reduce=True):
    """BN backward: dgamma / dbeta added to, dx written, the masked dy into dz_out (optional).
    part (fp32, bn_bwd_blocks(M, C) x 2C): reduce, finalize, apply (dx None: no apply).
    acc (int64 [reps + 1][4C]): reduce, then an apply that derives co and adds dgamma / dbeta.
    reduce=False: a conv epilogue (E_BNRED) already wrote part's rows / added into acc."""
    C = x.shape[-1]
    M = x.numel() // C
    red, fin = _bwd_stats(part, acc, M, C, co, dgamma, dbeta, "bn_bwd")
    by_acc = acc is not None
    T = bn_bwd_blocks(M, C) if reduce or by_acc else part.shape[0]
    s = stream_handle()
    if reduce:
        assert by_acc or part.numel() >= T * 2 * C
        _C().bn_bwd_reduce(_ptr(dy), _ptr(y), int(relu_mask), _ptr(x), _ptr(st), _ptr(dz_out), _ptr(part), T, M, C, s,
                           **red)
        if by_acc and dz_out is not None and relu_mask:
            # the reduce just wrote the masked gradient: the apply reads it instead of dy and
            # the mask source (one input tensor less, the same values)
            dy, y, relu_mask = dz_out, None, 0
    if not by_acc:
        _C().bn_bwd_finalize(_ptr(part), T, C, float(M), _ptr(st), _ptr(dgamma), _ptr(dbeta), _ptr(co), s)
    if by_acc or dx is not None:  # (the accumulator's apply is also its finalize)
        _C().bn_bwd_apply(_ptr(dy), _ptr(y), int(relu_mask), _ptr(x), _ptr(st), _ptr(co), _ptr(dx), M, C, s, **fin)


def bn_bwd_fin_dual(dy, y, relu_mask, bns):
    """Backward of two BatchNorms fed by the same (masked) gradient dy -- the two BN inputs
    of relu(BN(x) + BN(xd)) -- in two launches instead of four (bn_bwd_reduce_dual /
    bn_bwd_apply_dual: one read of dy and the mask source y for both, bitwise the single-BN
    launches).  Accumulators only.  bns: two dicts x, st, acc, co, dx, dgamma, dbeta."""
    a, b = bns
    C = a["x"].shape[-1]
    M = a["x"].numel() // C
    r = acc_reps(a["acc"], C, 4)
    if b["x"].shape != a["x"].shape or acc_reps(b["acc"], C, 4) != r or relu_mask not in (0, 1):
        raise ValueError("bn_bwd_fin_dual: the two BatchNorms must match in shape and replicas")
    T = bn_bwd_blocks(M, C)
    s = stream_handle()
    _C().bn_bwd_reduce_dual_acc(_ptr(dy), _ptr(y), int(relu_mask), _ptr(a["x"]), _ptr(b["x"]), _ptr(a["st"]),
                                _ptr(b["st"]), _ptr(a["acc"]), _ptr(b["acc"]), T, M, C, s, r)
    _C().bn_bwd_apply_dual_fin(_ptr(dy), _ptr(y), int(relu_mask), _ptr(a["x"]), _ptr(b["x"]), _ptr(a["st"]),
                               _ptr(b["st"]), _ptr(a["dx"]), _ptr(b["dx"]), M, C,
                               [_ptr(a["acc"]), _ptr(a.get("dgamma")), _ptr(a.get("dbeta")), _ptr(a["co"])],
                               [_ptr(b["acc"]), _ptr(b.get("dgamma")), _ptr(b.get("dbeta")), _ptr(b["co"])],
                               float(M), s, r)


def pool_geo(x_shape, pool, strides, padding):
    n, h, w, c = x_shape
    if padding == "same":
        ho, pt, _ = same_pad(h, pool[0], strides[0])
        wo, pl, _ = same_pad(w, pool[1], strides[1])
    else:
        ho, pt = (h - pool[0]) // strides[0] + 1, 0
        wo, pl = (w - pool[1]) // strides[1] + 1, 0
    return [n, h, w, c, pool[0], pool[1], strides[0], strides[1], pt, pl, ho, wo]


def maxpool_fwd(x, y, arg, pool, strides, padding):
    g = pool_geo(x.shape, pool, strides, padding)
    _C().maxpool_fwd(_ptr(x), g, _ptr(y), _ptr(arg), stream_handle())


def maxpool_bwd(dy, arg, dx, pool, strides, padding):
    g = pool_geo(dx.shape, pool, strides, padding)
    _C().maxpool_bwd(_ptr(dy), _ptr(arg), g, _ptr(dx), stream_handle())


def bn_relu_maxpool_fwd(x, st, y, arg, pool, strides, padding):
    """y, arg = maxpool(relu(BN(x))) without materialising the BN output (stem fusion); st: an
    fp32 [4][C] tensor or a BNFin."""
    g = pool_geo(x.shape, pool, strides, padding)
    s1, p, v = _fwd_stats(st)
    _C().bn_relu_maxpool_fwd(_ptr(x), s1, g, _ptr(y), _ptr(arg), stream_handle(), fin=p, fin_v=v)


def pool_bn_bwd(dpool, arg, x, st, part, co, dx, pool, strides, padding, dgamma=None, dbeta=None, acc=None):
    """Backward of bn_relu_maxpool_fwd: BN batch-statistics backward with the pool routing and
    ReLU mask recomputed; part / acc and the launches as bn_bwd's."""
    g = pool_geo(x.shape, pool, strides, padding)
    C = x.shape[-1]
    M = x.numel() // C
    red, fin = _bwd_stats(part, acc, M, C, co, dgamma, dbeta, "pool_bn_bwd")
    by_acc = acc is not None
    T = bn_bwd_blocks(M, C)
    assert by_acc or part.numel() >= T * 2 * C
    s = stream_handle()
    _C().pool_bn_bwd_reduce(_ptr(dpool), _ptr(arg), g, _ptr(x), _ptr(st), _ptr(part), T, s, **red)
    if not by_acc:
        _C().bn_bwd_finalize(_ptr(part), T, C, float(M), _ptr(st), _ptr(dgamma), _ptr(dbeta), _ptr(co), s)
    if by_acc or dx is not None:
        _C().pool_bn_bwd_apply(_ptr(dpool), _ptr(arg), g, _ptr(x), _ptr(st), _ptr(co), _ptr(dx), s, **fin)


# ---- other per-layer kernels, loss, optimizer ---------------------------------------------------
def gap_fwd(x, y):
    n, h, w, c = x.shape
    _C().gap_fwd(_ptr(x), n, h * w, c, _ptr(y), int(y.dtype == torch.float32), stream_handle())


def gap_bwd(dy, dx):
    n, h, w, c = dx.shape
    _C().gap_bwd(_ptr(dy), int(dy.dtype == torch.float32), n, h * w, c, _ptr(dx), stream_handle())


def relu_bwd(dy, y, dz):
    _C().relu_bwd(_ptr(dy), _ptr(y), _ptr(dz), dy.numel(), stream_handle())


ACT_KINDS = {"relu": 0, "sigmoid": 1, "tanh": 2}


def act_fwd(x, y, kind: str):
    """y = act(x) on bf16 tensors (in place allowed); kind relu / sigmoid / tanh."""
    _C().act_fwd(_ptr(x), _ptr(y), x.numel(), ACT_KINDS[kind], stream_handle())


def act_bwd(dy, y, dx, kind: str):
    """dx = dy * act'(y) from the stored activation output y."""
    _C().act_bwd(_ptr(dy), _ptr(y), _ptr(dx), dy.numel(), ACT_KINDS[kind], stream_handle())


def dropout(x, y, ctrl, seed: int, rate: float):
    """y = x * keep / (1 - rate); keep from (seed, ctrl step t, element) -- the same call on
    dy is the backward (see dropout_mask_reference)."""
    _C().dropout(_ptr(x), _ptr(y), x.numel(), _ptr(ctrl), int(seed) & 0xFFFFFFFF, float(rate), stream_handle())


def _mix32(h):
    h = h.astype(np.uint32)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def dropout_mask_reference(n: int, seed: int, t: int, rate: float) -> np.ndarray:
    """Host oracle of the dropout kernel's keep mask (bool [n]) at step t."""
    with np.errstate(over="ignore"):
        key = _mix32(np.array([(int(seed) + int(t) * 0x9E3779B9) & 0xFFFFFFFF], dtype=np.uint64))[0]
        j = np.arange(n, dtype=np.uint64).astype(np.uint32)
        h = _mix32((_mix32(j ^ key).astype(np.uint64) + int(key)) & 0xFFFFFFFF)
    thr = min(int(rate * 4294967296.0), 4294967295)
    return h >= np.uint32(thr)


# --- input augmentation (csrc/kernels/augment.hip; layer_ops.h has the contract) ---------------
AUG_MAX_STAGES = 8  # layer_ops.h AUG_MAX_STAGES
AUG_WORDS = 68  # layer_ops.h AugTable
AUG_FLIP, AUG_CROP, AUG_PAD = 1, 2, 3
AUG_DEFAULT_SEED = 0xA06D  # a layer with seed=None
AUG_LAYERS = ("ZeroPadding2D", "RandomCrop", "RandomFlip")
AUG_FLIP_MODES = {"horizontal": 1, "vertical": 2, "horizontal_and_vertical": 3}


def aug_seed(seed, position: int) -> int:
    """The effective 32-bit seed of an augmentation layer: its ``seed`` (a fixed default for
    None) mixed with its position among the model's layers, so two layers of one model draw
    independently.  Neither rank nor world size enter."""
    s0 = AUG_DEFAULT_SEED if seed is None else int(seed)
    return (s0 * 0x9E3779B1 + (int(position) + 1) * 0x85EBCA77) & 0xFFFFFFFF


def aug_draws(seed: int, t: int, g):
    """(h, h2): the two 32-bit draws of global batch slots ``g`` (array) at step ``t`` under the
    effective ``seed`` -- h = mix32(mix32(g ^ key) + key), h2 = mix32(h + key), key =
    mix32(seed + t * 0x9E3779B9): Dropout's counter hash with the slot as the counter."""
    g = np.asarray(g, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        key = int(_mix32(np.array([(int(seed) + int(t) * 0x9E3779B9) & 0xFFFFFFFF], dtype=np.uint64))[0])
        h = _mix32((_mix32(g ^ np.uint64(key)).astype(np.uint64) + np.uint64(key)) & np.uint64(0xFFFFFFFF))
        h2 = _mix32((h.astype(np.uint64) + np.uint64(key)) & np.uint64(0xFFFFFFFF))
    return h, h2


def aug_flip_bits(seed: int, t: int, g, mode: int = 3):
    """(left-right, up-down) flip decisions (bool arrays over ``g``): bits 31 and 30 of the
    first draw, each only where ``mode`` (AUG_FLIP_MODES) has the axis."""
    h, _ = aug_draws(seed, t, g)
    lr = (h >> np.uint32(31)).astype(bool) & bool(mode & 1)
    ud = ((h >> np.uint32(30)) & np.uint32(1)).astype(bool) & bool(mode & 2)
    return lr, ud


def aug_crop_offsets(seed: int, t: int, g, range_y: int, range_x: int):
    """(oy, ox) crop offsets (int64 arrays over ``g``) in [0, range_y) x [0, range_x): the two
    draws reduced modulo the ranges."""
    h, h2 = aug_draws(seed, t, g)
    return (h % np.uint32(range_y)).astype(np.int64), (h2 % np.uint32(range_x)).astype(np.int64)


def aug_stages(layers, seeds, h: int, w: int):
    """The stage list of a chain of ZeroPadding2D / RandomCrop / RandomFlip ``layers`` applied
    to an ``h`` x ``w`` image, and the output size: ([(kind, p0, p1, p2, p3, seed)], ho, wo)
    with the parameters of layer_ops.h.  ``seeds``: {id(layer): effective seed}
    (keras/layers.py augment_seeds)."""
    stages = []
    for l in layers:
        k = type(l).__name__
        if k == "ZeroPadding2D":
            (pt, pb), (pl, pr) = l.padding
            stages.append((AUG_PAD, int(pt), int(pb), int(pl), int(pr), 0))
            h, w = h + pt + pb, w + pl + pr
        elif k == "RandomCrop":
            if l.height > h or l.width > w:
                raise ValueError(f"RandomCrop({l.height}, {l.width}) of a {h} x {w} input: there is no resize path")
            stages.append((AUG_CROP, l.height, l.width, 0, 0, int(seeds[id(l)])))
            h, w = l.height, l.width
        elif k == "RandomFlip":
            stages.append((AUG_FLIP, AUG_FLIP_MODES[l.mode], 0, 0, 0, int(seeds[id(l)])))
        else:
            raise ValueError(f"aug_stages: layer {k}")
    return stages, h, w


def aug_table(stages) -> torch.Tensor:
    """``augment``'s stage table (layer_ops.h AugTable): int32 [AUG_WORDS] in HOST memory --
    the stage count, then 8 words per stage (kind, four parameters, seed).  The kernel takes
    it by value, as a kernel argument; a captured step holds its own copy."""
    if not 1 <= len(stages) <= AUG_MAX_STAGES:
        raise ValueError(f"aug_table: {len(stages)} stages (1 .. AUG_MAX_STAGES = {AUG_MAX_STAGES})")
    w = np.zeros(AUG_WORDS, dtype=np.int32)
    w[0] = len(stages)
    for i, st in enumerate(stages):
        w[4 + 8 * i:4 + 8 * i + 5] = st[:5]
        w[4 + 8 * i + 5:4 + 8 * i + 6] = np.array([st[5] & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)
    return torch.from_numpy(w)


def augment(x, y, labels, ctrl, table, training: bool):
    """y [B, Ho, Wo, Cp] = the augmented x [B, H, W, Cp] (bf16 NHWC, Cp a multiple of 4) under
    ``table`` (aug_table) at step ctrl.cur3 for slots ctrl.row0 + b; rows with labels[b] < 0
    come out zero.  ``training`` False: flips off, crops centred."""
    _chk(x, torch.bfloat16, "x")
    _chk(y, torch.bfloat16, "y")
    _chk(labels, torch.int32, "labels")
    _chk(ctrl, torch.int32, "ctrl")
    if _C().AUG_WORDS != AUG_WORDS or _C().AUG_MAX_STAGES != AUG_MAX_STAGES:
        raise RuntimeError("ops/hip.py AUG_WORDS / AUG_MAX_STAGES do not match the native build")
    if table.dtype != torch.int32 or table.is_cuda or table.numel() != AUG_WORDS or not table.is_contiguous():
        raise ValueError("augment: table must be aug_table's host int32 words")
    if x.dim() != 4 or y.dim() != 4 or x.shape[0] != y.shape[0] or x.shape[3] != y.shape[3]:
        raise ValueError(f"augment: x {tuple(x.shape)} / y {tuple(y.shape)} must be NHWC with one batch and pitch")
    if labels.numel() < x.shape[0] or ctrl.numel() < 32:
        raise ValueError("augment: labels must hold one entry per row and ctrl the 32-word block")
    B, h, w, cp = x.shape
    _C().augment(_ptr(x), _ptr(y), _ptr(labels), _ptr(ctrl), table.data_ptr(), B, h, w, y.shape[1], y.shape[2], cp,
                 int(bool(training)), stream_handle())


def augment_reference(x_nhwc, stages, t: int, g0: int, training: bool) -> np.ndarray:
    """Host oracle of ``augment``: the batch ``x_nhwc`` (array [B, H, W, C], any dtype) after
    ``stages`` (aug_stages) at step ``t``, row b being global batch slot ``g0 + b``.  Values
    are only moved or replaced by zero, so the result is exact in x's dtype."""
    x = np.asarray(x_nhwc)
    g = np.arange(x.shape[0], dtype=np.int64) + int(g0)
    for kind, p0, p1, p2, p3, seed in stages:
        B, h, w = x.shape[:3]
        if kind == AUG_FLIP:
            if training:
                lr, ud = aug_flip_bits(seed, t, g, p0)
                x = np.where(lr[:, None, None, None], x[:, :, ::-1], x)
                x = np.where(ud[:, None, None, None], x[:, ::-1], x)
        elif kind == AUG_CROP:
            if p0 > h or p1 > w:
                raise ValueError(f"augment_reference: crop {p0} x {p1} of a {h} x {w} input")
            if training:
                oy, ox = aug_crop_offsets(seed, t, g, h - p0 + 1, w - p1 + 1)
            else:
                oy, ox = np.full(B, (h - p0) // 2), np.full(B, (w - p1) // 2)
            x = np.stack([x[b, oy[b]:oy[b] + p0, ox[b]:ox[b] + p1] for b in range(B)])
        elif kind == AUG_PAD:
            x = np.pad(x, ((0, 0), (p0, p1), (p2, p3), (0, 0)))
        else:
            raise ValueError(f"augment_reference: stage kind {kind}")
    return np.ascontiguousarray(x)


def avgpool_fwd(x, y, pool, strides, padding):
    g = pool_geo(x.shape, pool, strides, padding)
    _C().avgpool_fwd(_ptr(x), g, _ptr(y), stream_handle())


def avgpool_bwd(dy, dx, pool, strides, padding):
    g = pool_geo(dx.shape, pool, strides, padding)
    _C().avgpool_bwd(_ptr(dy), g, _ptr(dx), stream_handle())


# --- depthwise convolution (csrc/kernels/dwconv.hip), depth_multiplier 1 -----------------------
# geo: the pool_geo(x.shape, kernel_size, strides, padding) list; w: the bf16 taps of the
# depthwise kernel, [kh, kw, C, 1] or any view of kh * kw * C contiguous elements.
DWCONV_MAX_K = 7


def _dw_geo(geo, who):
    n, h, w, c, kh, kw, sh, sw, pt, pl, ho, wo = geo
    if c % 8:
        raise ValueError(f"{who}: channels must be a multiple of 8")
    return (n, h, w, c), (n, ho, wo, c), kh * kw * c


def dwconv_fwd(x, w, bias, relu, geo, y):
    """y [N,Ho,Wo,C] = bf16(act(depthwise conv of x [N,H,W,C] with taps w + bias)); bias fp32
    [C] or None, act the identity or ReLU."""
    xs, ys, nw = _dw_geo(geo, "dwconv_fwd")
    _chk(x, torch.bfloat16, "x")
    _chk(w, torch.bfloat16, "w")
    _chk(y, torch.bfloat16, "y")
    if bias is not None:
        _chk(bias, torch.float32, "bias")
        if bias.numel() != xs[3]:
            raise ValueError("dwconv_fwd: bias must hold C values")
    if tuple(x.shape) != xs or tuple(y.shape) != ys or w.numel() != nw:
        raise ValueError(f"dwconv_fwd: x {tuple(x.shape)}, w {tuple(w.shape)}, y {tuple(y.shape)} against geometry "
                         f"{geo}")
    _C().dwconv_fwd(_ptr(x), _ptr(w), _ptr(bias), int(bool(relu)), list(geo), _ptr(y), stream_handle())


def dwconv_dgrad(dy, w, geo, dx):
    """dx [N,H,W,C] = the backprop-input of dwconv_fwd; every element is written."""
    xs, ys, nw = _dw_geo(geo, "dwconv_dgrad")
    _chk(dy, torch.bfloat16, "dy")
    _chk(w, torch.bfloat16, "w")
    _chk(dx, torch.bfloat16, "dx")
    if tuple(dx.shape) != xs or tuple(dy.shape) != ys or w.numel() != nw:
        raise ValueError(f"dwconv_dgrad: dy {tuple(dy.shape)}, w {tuple(w.shape)}, dx {tuple(dx.shape)} against "
                         f"geometry {geo}")
    _C().dwconv_dgrad(_ptr(dy), _ptr(w), list(geo), _ptr(dx), stream_handle())


def dwconv_wgrad_workspace_elems(geo) -> int:
    """fp32 workspace floats of dwconv_wgrad: one partial row [kh * kw * C] per pixel slab."""
    return _C().dwconv_wgrad_blocks(list(geo)) * geo[4] * geo[5] * geo[3]


def dwconv_wgrad(x, dy, geo, dw, workspace=None):
    """dw (fp32, kh * kw * C elements) += sum over the output pixels of x * dy, in a fixed
    order (no float atomics): repeated launches give the same bits."""
    xs, ys, nw = _dw_geo(geo, "dwconv_wgrad")
    _chk(x, torch.bfloat16, "x")
    _chk(dy, torch.bfloat16, "dy")
    _chk(dw, torch.float32, "dw")
    if geo[4] != geo[5] or geo[4] > DWCONV_MAX_K:
        raise ValueError(f"dwconv_wgrad: square kernels up to {DWCONV_MAX_K} x {DWCONV_MAX_K}")
    if tuple(x.shape) != xs or tuple(dy.shape) != ys or dw.numel() != nw:
        raise ValueError(f"dwconv_wgrad: x {tuple(x.shape)}, dy {tuple(dy.shape)}, dw {tuple(dw.shape)} against "
                         f"geometry {geo}")
    ws = _workspace(workspace, dwconv_wgrad_workspace_elems(geo), x.device)
    _C().dwconv_wgrad(_ptr(x), _ptr(dy), list(geo), _ptr(dw), _ptr(ws), stream_handle())


def add_bf16(a, b, out):
    _C().add_bf16(_ptr(a), _ptr(b), _ptr(out), a.numel(), stream_handle())


def colsum_workspace_elems(M: int, N: int) -> int:
    """fp32 workspace floats colsum needs for an [M][N] input (0: one pass, no workspace)."""
    sp = _C().colsum_splits(M, N)
    return sp * N if sp > 1 else 0


def colsum(x, out, workspace=None, M=None, N=None, ld=None):
    """out[n] += sum over rows of x (bf16 or fp32) in a fixed order (no float atomics)."""
    N = N or x.shape[-1]
    ld = ld or N
    M = M or x.numel() // ld
    need = colsum_workspace_elems(M, N)
    if need and (workspace is None or workspace.numel() < need):
        workspace = torch.empty(need, dtype=torch.float32, device=x.device)  # (eager callers only)
    _C().colsum(_ptr(x), int(x.dtype == torch.float32), M, N, ld, _ptr(out), stream_handle(),
                _ptr(workspace) if need else 0)


def xent_rows(B: int, device) -> torch.Tensor:
    """softmax_xent's per-row scratch: 3 B floats + the arrival counter (zeroed once)."""
    return torch.zeros(3 * B + 1, dtype=torch.float32, device=device)


def _chk_loss_weights(weights, B, ctrl, where):
    """Per-row loss weights: fp32, contiguous, 1-D; one per logits row without ``ctrl`` (with
    it the kernel indexes the epoch-ordered array at the device cursor)."""
    if weights.dtype != torch.float32:
        raise ValueError(f"{where}: weights must be float32, got {weights.dtype}")
    if weights.dim() != 1 or not weights.is_contiguous():
        raise ValueError(f"{where}: weights must be a contiguous 1-D tensor")
    if not weights.is_cuda:
        raise ValueError(f"{where}: weights must be a device tensor")
    if ctrl is None and weights.numel() < B:
        raise ValueError(f"{where}: {B} logits rows but {weights.numel()} weights")


def softmax_xent(logits, labels, K, scale, dlogits, tail, ctrl=None, rows=None, bias_grad=None, weights=None):
    """ctrl (the engine's device control block) makes the scale 1 / real rows of the global
    batch; labels < 0 mark padding rows of a short final batch.  The loss / correct / count
    sums are formed in a fixed row order (``rows``: :func:`xent_rows` scratch).
    ``bias_grad`` (fp32 [K], optional; needs :func:`softmax_bias_fold_ok`): += the column
    sums of dlogits, bitwise as :func:`colsum` would add them.
    ``weights`` (fp32, optional): a row's dlogits and loss are multiplied by its weight, the
    correct / count sums are not.  Without ``ctrl`` row b has ``weights[b]``; with it the
    weight of the sample at the device cursor, ``weights[cursor * global_batch + row0 + b]``
    (modulo nsamples in wrap mode).  A row with label < 0 never reads the array."""
    B, ld = logits.shape
    if weights is not None:
        _chk_loss_weights(weights, B, ctrl, "softmax_xent")
    if rows is None:
        rows = xent_rows(B, logits.device)  # (eager callers only: engines pass their own)
    if bias_grad is not None:
        _chk(bias_grad, torch.float32, "bias_grad")
        if bias_grad.numel() < K or not softmax_bias_fold_ok(B, K):
            raise ValueError("softmax_xent: bias_grad needs >= K floats and a one-split colsum shape")
    _C().softmax_xent(_ptr(logits), ld, _ptr(labels), B, K, float(scale), _ptr(ctrl), _ptr(dlogits), _ptr(tail),
                      _ptr(rows), stream_handle(), bias_grad=_ptr(bias_grad), weights=_ptr(weights))


def softmax_xent_dense(logits, targets, K, scale, dlogits, tail, label_smoothing=0.0, labels=None, ctrl=None,
                       rows=None, bias_grad=None, weights=None):
    """:func:`softmax_xent` against dense fp32 target rows ``[n, K]`` (one-hot or soft) with
    Keras label smoothing: loss = -sum y' log softmax, dlogits = (softmax * sum y' - y') *
    scale, correct = argmax logits == argmax targets.  Without ``ctrl`` row b of ``targets``
    belongs to logits row b; with ``ctrl`` the kernel reads row ``cursor * global_batch +
    row0 + b`` of the epoch-ordered targets (modulo nsamples in wrap mode) and ``labels``
    (int32 [B], >= 0 real / < 0 past the end of the data) is required.  ``weights``: as
    :func:`softmax_xent`, indexed by the target row."""
    B, ld = logits.shape
    if weights is not None:
        _chk_loss_weights(weights, B, ctrl, "softmax_xent_dense")
    _chk(logits, torch.float32, "logits")
    _chk(targets, torch.float32, "targets")
    if targets.dim() != 2 or targets.shape[1] != K:
        raise ValueError(f"softmax_xent_dense: targets must be [n, {K}], got {tuple(targets.shape)}")
    if K > ld or tuple(dlogits.shape) != (B, ld):
        raise ValueError("softmax_xent_dense: dlogits must share the logits' shape and K <= row pitch")
    _chk(dlogits, torch.bfloat16, "dlogits")
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError(f"softmax_xent_dense: label_smoothing {label_smoothing} not in [0, 1)")
    if ctrl is None and targets.shape[0] < B:
        raise ValueError(f"softmax_xent_dense: {B} logits rows but {targets.shape[0]} target rows")
    if labels is not None:
        _chk(labels, torch.int32, "labels")
        if labels.numel() < B:
            raise ValueError("softmax_xent_dense: labels needs one entry per logits row")
    elif ctrl is not None:
        raise ValueError("softmax_xent_dense: ctrl addressing needs the step's labels (row validity)")
    if rows is None:
        rows = xent_rows(B, logits.device)  # (eager callers only: engines pass their own)
    if bias_grad is not None:
        _chk(bias_grad, torch.float32, "bias_grad")
        if bias_grad.numel() < K or not softmax_bias_fold_ok(B, K):
            raise ValueError("softmax_xent_dense: bias_grad needs >= K floats and a one-split colsum shape")
    _C().softmax_xent_dense(_ptr(logits), ld, _ptr(labels), _ptr(targets), B, K, float(label_smoothing), float(scale),
                            _ptr(ctrl), _ptr(dlogits), _ptr(tail), _ptr(rows), stream_handle(),
                            bias_grad=_ptr(bias_grad), weights=_ptr(weights))


def softmax_store(logits, K, ctrl, out):
    """out[global row] = softmax(logits row) for the rows of the step at the device cursor
    (``ctrl``) that exist; ``out`` is fp32 ``[n, K]`` with n >= ctrl's nsamples."""
    B, ld = logits.shape
    _chk(logits, torch.float32, "logits")
    _chk(out, torch.float32, "out")
    _chk(ctrl, torch.int32, "ctrl")
    if K > ld or out.dim() != 2 or out.shape[1] != K:
        raise ValueError(f"softmax_store: out must be [n, {K}] and K <= the logits' row pitch {ld}")
    if ctrl.numel() < 32:
        raise ValueError("softmax_store: ctrl is the 32-word device control block")
    _C().softmax_store(_ptr(logits), ld, K, B, _ptr(ctrl), _ptr(out), stream_handle())


def softmax_bias_fold_ok(B: int, K: int) -> bool:
    """colsum of a [B][K] gradient runs as one split (the order softmax_xent reproduces)."""
    return _C().colsum_splits(B, K) == 1


def sgd_flat(P, G, V, Pb, lr, momentum=0.0, nesterov=False):
    _C().sgd_flat(_ptr(P), _ptr(G), _ptr(V), _ptr(Pb), P.numel(), float(lr), float(momentum), int(nesterov),
                  stream_handle())


REG_MAX_ROWS = 2048  # layer_ops.h REG_MAX_ROWS: the segment table is staged whole into LDS


def reg_table(rows, device) -> torch.Tensor:
    """The weight-regularizer segment table of ``opt_step`` / ``reg_penalty`` on the device:
    int32 [nreg, 4] rows (offset, size, l1 as float bits, l2 as float bits) from host rows
    ``(offset, size, l1, l2)``, sorted by offset.  Offsets index the flat parameter buffer
    and must be multiples of 8 (the padding behind a variable is zero); rows may not overlap."""
    rows = sorted((int(o), int(n), float(a), float(b)) for o, n, a, b in rows)
    if len(rows) > REG_MAX_ROWS:
        raise ValueError(f"reg_table: {len(rows)} rows exceed the table cap {REG_MAX_ROWS}")
    end = 0
    for o, n, _, _ in rows:
        if o % 8 or n <= 0 or o < end:
            raise ValueError(f"reg_table: row (offset {o}, size {n}) is misaligned, empty or overlaps the previous")
        end = o + n
    if end >= 2 ** 31:
        raise ValueError("reg_table: offsets are 32-bit (a flat buffer below 2^31 elements)")
    t = torch.zeros((max(len(rows), 1), 4), dtype=torch.int32)
    if rows:
        t[:len(rows), :2] = torch.tensor([r[:2] for r in rows], dtype=torch.int32)
        t[:len(rows), 2:] = torch.tensor([r[2:] for r in rows], dtype=torch.float32).view(torch.int32)
    return t.to(device)[:len(rows)]


def reg_scratch(n: int, device) -> torch.Tensor:
    """reg_penalty's scratch for a flat buffer of n floats: per-block partials, the arrival
    counter (zeroed once; every launch re-arms it) and R, the last word."""
    return torch.zeros(_C().reg_penalty_blocks(int(n)) + 2, dtype=torch.float32, device=device)


def _chk_reg(P, table, where):
    _chk(P, torch.float32, "P")
    _chk(table, torch.int32, "table")
    if table.dim() != 2 or table.shape[1] != 4 or table.shape[0] > REG_MAX_ROWS:
        raise ValueError(f"{where}: table must be int32 [nreg <= {REG_MAX_ROWS}, 4] (reg_table)")


def reg_penalty(P, table, scratch, tail=None):
    """R = sum over the table's rows of l1 sum|w| + l2 sum(w^2) over the flat fp32 buffer
    ``P``, in a fixed order; stored in ``scratch[-1]`` (read it after a sync) and, with
    ``tail``, ``tail[0] += R * tail[2]``.  A table without rows launches nothing (R = 0)."""
    _chk_reg(P, table, "reg_penalty")
    n = P.numel()
    if n % 4:
        raise ValueError("reg_penalty: the flat buffer must hold a multiple of 4 floats")
    _chk(scratch, torch.float32, "scratch")
    if scratch.numel() != _C().reg_penalty_blocks(n) + 2:
        raise ValueError("reg_penalty: scratch must come from reg_scratch(P.numel())")
    if tail is not None:
        _chk(tail, torch.float32, "tail")
        if tail.numel() < 3:
            raise ValueError("reg_penalty: tail holds [loss sum, correct, count, ...]")
    if table.shape[0] == 0:
        scratch[-1:].zero_()
        return
    _C().reg_penalty(_ptr(P), n, _ptr(table), table.shape[0], _ptr(scratch), _ptr(tail), stream_handle())


GN_CHUNK = 4096  # layer_ops.h GN_CHUNK: elements per chunk of grad_norm's partition
CLIP_KINDS = {None: 0, "clipvalue": 1, "clipnorm": 2, "global_clipnorm": 3}  # opt_step's clip argument


class ClipPlan:
    """Device tables and buffers of ``grad_norm`` for one flat-buffer layout (built once: a
    captured step replays with no allocation).  ``vt`` int32 [nvar, 4]: one row (offset,
    size, l1 bits, l2 bits) per variable -- also opt_step's table for per-variable clipping;
    ``ct`` int32 [nchunk, 2]: (start, row) of every chunk; ``vfirst`` int32 [nvar + 1]: each
    variable's first chunk; ``scratch`` fp32 [nchunk + 1]; ``out`` fp32 [2, nout]: the norms
    and the scales (``nout`` = nvar per variable, 1 for the global norm)."""

    def __init__(self, rows, n: int, device, per_variable: bool):
        rows = [(int(r[0]), int(r[1]), float(r[2]) if len(r) > 2 else 0.0, float(r[3]) if len(r) > 3 else 0.0)
                for r in rows]
        if rows != sorted(rows) or not rows:
            raise ValueError("clip_plan: rows must be sorted by offset and not empty")
        n = int(n)
        if n % 4 or n >= 2 ** 31:
            raise ValueError("clip_plan: the flat buffer holds a multiple of 4 floats, below 2^31")
        end = 0
        for o, sz, _, _ in rows:
            if o % 8 or sz <= 0 or o < end or o + sz > n:
                raise ValueError(f"clip_plan: row (offset {o}, size {sz}) is misaligned, empty, overlaps the "
                                 f"previous or runs past the buffer ({n})")
            end = o + sz
        if per_variable and len(rows) > REG_MAX_ROWS:
            raise ValueError(f"clip_plan: {len(rows)} variables exceed the table cap {REG_MAX_ROWS}")
        chunks, first = [], []
        for r, (o, sz, _, _) in enumerate(rows):
            first.append(len(chunks))
            chunks += [(s, r) for s in range(o, o + sz, GN_CHUNK)]
        first.append(len(chunks))
        self.n, self.per_variable, self.rows = n, bool(per_variable), rows
        self.nvar, self.nchunk = len(rows), len(chunks)
        self.regularized = any(a or b for _, _, a, b in rows)
        vt = torch.zeros((self.nvar, 4), dtype=torch.int32)
        vt[:, :2] = torch.tensor([r[:2] for r in rows], dtype=torch.int32)
        vt[:, 2:] = torch.tensor([r[2:] for r in rows], dtype=torch.float32).view(torch.int32)
        self.vt = vt.to(device)
        self.ct = torch.tensor(chunks, dtype=torch.int32).to(device)
        self.vfirst = torch.tensor(first, dtype=torch.int32).to(device)
        self.scratch = torch.zeros(self.nchunk + 1, dtype=torch.float32, device=device)
        self.nout = self.nvar if per_variable else 1
        self.out = torch.zeros((2, self.nout), dtype=torch.float32, device=device)

    @property
    def norms(self):
        return self.out[0]

    @property
    def scales(self):
        return self.out[1]

    @property
    def bytes_read(self):
        """Bytes of G (and P) one launch loads."""
        g = sum(4 * ((sz + 3) // 4 * 4) for _, sz, _, _ in self.rows)
        p = sum(4 * ((sz + 3) // 4 * 4) for _, sz, a, b in self.rows if a or b)
        return g + p


def clip_plan(rows, n, device, per_variable) -> ClipPlan:
    """:class:`ClipPlan` for variables ``rows`` = (offset, size[, l1, l2]) sorted by offset
    (offsets multiples of 8, no overlap) in a flat buffer of ``n`` floats."""
    if _C().GN_CHUNK != GN_CHUNK:
        raise RuntimeError("ops/hip.py GN_CHUNK does not match the native build")
    return ClipPlan(rows, n, device, per_variable)


def grad_norm(G, plan: ClipPlan, c, P=None):
    """One launch: the L2 norm(s) of ``G`` over ``plan``'s variables -- with ``P`` (the fp32
    masters) of ``G + 2 l2 w + l1 sign(w)``, opt_step's regularized gradient -- into
    ``plan.norms`` and the clipping scales ``c / max(norm, c)`` into ``plan.scales``.  ``G``
    may be longer than the plan's buffer (a metric tail); the padding between variables
    must be zero in ``G`` and ``P``."""
    _chk(G, torch.float32, "G")
    if G.numel() < plan.n:
        raise ValueError(f"grad_norm: G holds {G.numel()} floats, the plan covers {plan.n}")
    if P is not None:
        _chk(P, torch.float32, "P")
        if P.numel() < plan.n:
            raise ValueError(f"grad_norm: P holds {P.numel()} floats, the plan covers {plan.n}")
    elif plan.regularized:
        raise ValueError("grad_norm: the plan has regularizer coefficients: pass the masters P")
    c = float(c)
    if not (math.isfinite(c) and c > 0.0):
        raise ValueError(f"grad_norm: c must be a finite number > 0, got {c}")
    _C().grad_norm(_ptr(G), _ptr(P) if plan.regularized else 0, plan.n, _ptr(plan.vt), plan.nvar, _ptr(plan.ct),
                   plan.nchunk, _ptr(plan.vfirst), int(plan.per_variable), c, _ptr(plan.scratch), _ptr(plan.out),
                   stream_handle())


LR_MAX_BOUNDS = 16  # layer_ops.h LR_MAX_BOUNDS: boundaries of a PiecewiseConstantDecay in the descriptor
LR_MAX_STEPS = 1 << 24  # layer_ops.h LR_MAX_STEPS: decay_steps / warmup_steps, exact as a float
LR_WORDS = 44  # layer_ops.h LrSched
LR_KINDS = {"ExponentialDecay": 1, "InverseTimeDecay": 2, "PolynomialDecay": 3, "PiecewiseConstantDecay": 4,
            "CosineDecay": 5}  # layer_ops.h LR_*


def lr_schedule_ok(schedule):
    """(ok, reason): ``schedule`` fits ``opt_step``'s descriptor -- exactly one of the five
    keras/schedules.py classes, integral ``decay_steps`` in [1, 2^24] and ``warmup_steps`` in
    [0, 2^24], integer boundaries (at most LR_MAX_BOUNDS, within int32), finite parameters."""
    name = type(schedule).__name__
    from ..keras import schedules as S

    if type(schedule) is not getattr(S, name, None) or name not in LR_KINDS:
        return False, f"learning-rate schedule {name}"
    why = f"learning-rate schedule {name}: "

    def integral(v, lo, hi):
        return isinstance(v, int) and not isinstance(v, bool) and lo <= v <= hi

    floats = []
    if name == "PiecewiseConstantDecay":
        if len(schedule.boundaries) > LR_MAX_BOUNDS:
            return False, (f"learning-rate schedule: {len(schedule.boundaries)} boundaries exceed the table cap "
                           f"{LR_MAX_BOUNDS}")
        if not all(integral(b, -2 ** 31, 2 ** 31 - 1) for b in schedule.boundaries):
            return False, why + "boundaries are not 32-bit integers"
        floats = list(schedule.values)
    else:
        if not integral(schedule.decay_steps, 1, LR_MAX_STEPS):
            return False, why + f"decay_steps {schedule.decay_steps!r} is not an integer in [1, 2^24]"
        floats = [schedule.initial_learning_rate]
        if name in ("ExponentialDecay", "InverseTimeDecay"):
            floats.append(schedule.decay_rate)
        elif name == "PolynomialDecay":
            floats += [schedule.end_learning_rate, schedule.power]
        else:
            floats.append(schedule.alpha)
            if schedule.warmup_target is not None:
                floats.append(schedule.warmup_target)
                if not integral(schedule.warmup_steps, 0, LR_MAX_STEPS):
                    return False, why + f"warmup_steps {schedule.warmup_steps!r} is not an integer in [0, 2^24]"
    if not all(math.isfinite(f) and abs(f) <= 3.4028234663852886e38 for f in floats):
        return False, why + "a parameter is not a finite float32"
    return True, ""


def lr_table(schedule, device=None) -> torch.Tensor:
    """``opt_step``'s learning-rate schedule descriptor (layer_ops.h LrSched): int32
    [LR_WORDS] -- kind, flags, decay_steps, warmup_steps, three float parameters as bits, the
    number of boundaries, LR_MAX_BOUNDS boundaries, LR_MAX_BOUNDS + 1 values as bits.  The
    kernel takes it by value, as a kernel argument, so it lives in HOST memory whatever
    ``device`` the step runs on (torch allocates it 64-byte aligned); keep the tensor alive
    for the call only -- a captured step holds its own copy."""
    ok, why = lr_schedule_ok(schedule)
    if not ok:
        raise ValueError(f"lr_table: {why}")
    if _C().LR_WORDS != LR_WORDS or _C().LR_MAX_BOUNDS != LR_MAX_BOUNDS:
        raise RuntimeError("ops/hip.py LR_WORDS / LR_MAX_BOUNDS do not match the native build")
    name = type(schedule).__name__
    w = np.zeros(LR_WORDS, dtype=np.int32)
    f = w.view(np.float32)
    w[0] = LR_KINDS[name]
    if name == "PiecewiseConstantDecay":
        nb = len(schedule.boundaries)
        w[7] = nb
        w[8:8 + nb] = schedule.boundaries
        f[24:24 + nb + 1] = schedule.values
    else:
        w[2] = schedule.decay_steps
        f[4] = schedule.initial_learning_rate
        if name in ("ExponentialDecay", "InverseTimeDecay"):
            w[1], f[5] = int(schedule.staircase), schedule.decay_rate
        elif name == "PolynomialDecay":
            w[1], f[5], f[6] = int(schedule.cycle), schedule.end_learning_rate, schedule.power
        else:
            f[5] = schedule.alpha
            if schedule.warmup_target is not None:
                w[1], w[3], f[6] = 1, schedule.warmup_steps, schedule.warmup_target
    return torch.from_numpy(w)


def cast_bf16(x, y):
    _C().cast_f32_bf16(_ptr(x), _ptr(y), x.numel(), stream_handle())


def pad_cast(src, R, C1, C2, C1p, C2p, dst):
    _C().pad_cast(_ptr(src), R, C1, C2, C1p, C2p, _ptr(dst), stream_handle())


def unpad_add(src, R, C1, C2, C1p, C2p, dst):
    _C().unpad_add(_ptr(src), R, C1, C2, C1p, C2p, _ptr(dst), stream_handle())
