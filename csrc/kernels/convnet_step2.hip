// Two-launch data-parallel training step for the reference MNIST CNN (gfx950 / MI355X).
//
// Model (reference README.md:58-73): Conv2D(32,3x3,valid)+bias+ReLU
// -> MaxPool 2x2 -> Flatten(NHWC, 5408) -> Dense(64)+bias+ReLU -> Dense(10) ->
// SparseCategoricalCrossentropy(from_logits); SGD(lr, momentum, nesterov) on fp32 masters.
//
// Why two launches: at B = 64 the step is a chain of dependent memory round trips, and
// every launch costs ~2.5-3 us of prologue latency plus ~2.8 us of drain + dispatch
// (profiles/r02_mnist phase stamps).  The 3-launch step (convnet_fused.hip) needed its
// middle kernel only to combine the 57 dense-1 split-K slabs per row; here those partial
// sums, and the conv-gradient partials, are combined by integer atomics on fixed-point
// values, so the combine needs no extra launch and -- unlike fp32 atomics -- its result
// does not depend on arrival order: every step is bitwise reproducible.
//
//   fwd (grid NS slices x IG image groups, 512 thr; 768 in the flagship configuration, see
//       CfgFlagFwd): the pending SGD update of the W1
//       slice and of the conv parameters (both double-buffered by step parity: every
//       block updates in registers, one owner block writes the next buffer) and of
//       b1/W2/b2 (two owner blocks); conv + bias + ReLU + 2x2 max-pool on MFMA (pooled
//       tile + argmax codes stored for bwd); the dense-1 partial of the slice on MFMA,
//       added into hacc[par][row][n] as round(v * 2^32) with 64-bit atomics.
//   bwd (grid NS slices, 512 thr; 1024 in the flagship configuration, one dh / dW1 / dP tile
//       per wave and the conv gradient split by taps, see CfgFlagBwd): every block converts
//       hacc back, adds b1, and runs the
//       whole head redundantly: Dense(10) logits on f32 MFMA (16x16x4, exact fp32) with
//       softmax-xent / accuracy / dz by 16-lane shuffles in the same waves, dh as a bf16
//       hi+lo pair in both MFMA operand layouts in LDS (no global round trip for dh), its
//       share of the b1/W2/b2 gradient and of the metric tail (fixed row order);
//       dW1 = P^T dh and dP = dh W1^T on MFMA; MaxPool/ReLU backward through the stored
//       argmax codes fused into this slice's conv weight-gradient partial, added into
//       hconv[par] as round(v * 2^40) with 64-bit atomics; the dead parity of hacc is
//       zeroed for the next step.
//       In the flagship configuration the two groups of work behind dh run on separate
//       blocks (grid 2 NS, a role per block, see CfgFlagBwd::SPLIT): the conv role -- dP, the
//       conv gradient, the hconv atomics -- is the kernel's critical chain; the W1 role --
//       dW1, the eager update and its 2.1 MB of stores, the aux sums, the zeroing, the
//       next-batch rows -- ends earlier, on CUs that used to idle.  Both run the head.
//   The bf16 copy of W1 that fwd (dense-1) and bwd (dP) read has one buffer per step parity:
//   a step of parity p reads buffer p, bwd's eager update writes buffer p ^ 1 (see below).
//   No block waits on another: there is no ticket / last-arriver hand-off inside either
//   launch (a returning atomic on a contended counter stalled its wave ~1.5-2 us), and no
//   block reads what another block of the same launch writes.
//
// Fixed point: h partials are fp32 MFMA sums of |v| < 2^31; x 2^32 keeps every bit a
// float carries down to 2^-32 (the sum of 57 roundings is < 1.4e-8 absolute); conv
// gradient partials x 2^40 (resolution 9e-13, range 8e6).  Integer addition is
// associative, so ranks and replays agree bitwise; the all-reduce sums both int64
// parities exactly too (the dead one is re-zeroed before its next use).
//
// Step counter / parity without intra-kernel races: fwd block 0 copies ctrl.cursor and
// ctrl.wpar to cur2 / par2; bwd reads those and its block 0 advances cursor / iterations,
// flips wpar and sets `pending`; no kernel uses a ctrl field that the same kernel writes.
#include "convnet_dev.h"

// Timing probes (wrong numerics, never in a product build): a probe build compiles this
// file with -DDAMD_PROBE_HACC=1|2 (skip all / half of the dense-1 atomics) or
// -DDAMD_PROBE_HCONV=1 (skip the conv-gradient atomics); scripts/probe_build.py makes one
// in a scratch directory.  The default build has both at 0, so the branches fold away.
#ifndef DAMD_PROBE_HACC
#define DAMD_PROBE_HACC 0
#endif
#ifndef DAMD_PROBE_HCONV
#define DAMD_PROBE_HCONV 0
#endif

namespace damd {
namespace convnet2 {
using namespace convnet;

constexpr int NAUX2 = NSMALL + 3;               // b1/W2/b2 gradients + [loss, correct, count]
constexpr int HPITCH = HID + 1;                 // fp32 pitch of the h tile in LDS
constexpr int ZP = 17;                          // pitch of the logit / dz rows (16 lanes store, odd: no conflicts)
constexpr int HEAD_FLOATS = CH * HPITCH + 716 + CH * ZP + 2 * CH + 16 * HID + CH;
constexpr int HEAD_BYTES = HEAD_FLOATS * 4;

// ---- sharded multi-rank exchange (XArgs, convnet.h) ----------------------------------
// Flag words live in every rank's uncached `out` staging; a flag holds the exchange epoch
// E (ctrl.xcnt after the step's bwd) of the last message it announces.  Publish: a wave
// drains its stores (s_waitcnt vmcnt(0): uncached stores are acknowledged by the owning
// device's memory) and one lane stores E with a relaxed system-scope atomic.  Consume: a
// lane polls with relaxed system-scope loads; the data loads follow in program order
// (uncached: nothing stale in any L1 / L2).  Every wait is bounded: on expiry the status
// word records which kind of wait expired and the kernel goes on (no GPU hang; the host
// raises on a non-zero status).
constexpr int SM_CONV = 0, SM_GRAD = 2 * NCONV, SM_MET = SM_GRAD + NSMALL;  // small-message fields
static_assert(SM_MET + 3 <= kXSmsg, "small message");
__device__ __forceinline__ unsigned* x_flags(float* out) { return reinterpret_cast<unsigned*>(out + kXFlags); }
__device__ __forceinline__ unsigned* x_pflag(float* out, int u, int slot) {
  return x_flags(out) + u * kXPFlagPitch + slot;
}
__device__ __forceinline__ unsigned* x_gflag(float* out, int nu, int u, int half) {
  return x_flags(out) + nu * kXPFlagPitch + u * 2 + half;
}
__device__ __forceinline__ unsigned* x_sflag(float* out, int nu, int par, int src) {
  return x_flags(out) + nu * (kXPFlagPitch + 2) + par * kXMaxRanks + src;
}
__device__ __forceinline__ float* x_small(float* out, int par, int src) {
  return out + kXSmall + ((long)par * kXMaxRanks + src) * kXSmsg;
}
__device__ __forceinline__ void x_signal(unsigned* f, unsigned e) {
  __hip_atomic_store(f, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void x_wait(const XArgs& xa, unsigned* f, unsigned e, unsigned bit) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < e) {
    __builtin_amdgcn_s_sleep(1);
    const unsigned long long dt = __builtin_amdgcn_s_memrealtime() - t0;
    if (dt > xa.timeout_ticks) {
      __hip_atomic_fetch_or(xa.status, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
    // past 1 ms: give up at once when an earlier wait already expired (a broken exchange
    // costs one deadline, not one per wait of every later step; the host raises on status)
    if (dt > 100000ull && __hip_atomic_load(xa.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
  }
}
constexpr unsigned XW_SMALL = 1u << 8, XW_UNIT = 1u << 9, XW_PART = 1u << 10;  // status bits
__device__ __forceinline__ uint2 pack_bf16x4(const f32x4& v) {
  return make_uint2((uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16),
                    (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16));
}
__device__ __forceinline__ float4 unpack_bf16x4(uint2 q) {
  return make_float4(bf2f((uint16_t)(q.x & 0xffffu)), bf2f((uint16_t)(q.x >> 16)), bf2f((uint16_t)(q.y & 0xffffu)),
                     bf2f((uint16_t)(q.y >> 16)));
}

// ---- compile-time configurations of the two step kernels -----------------------------
// PP = 0: every size is a runtime value (the generic kernels: any B, any slicing, chunked
// backward, deferred update, sharded exchange).  PP > 0: the sizes of one configuration are
// constants -- LDS pitches and offsets become immediates, the slice loops have constant trip
// counts and unroll, and the code of the paths the configuration never takes (deferred
// update, sharded exchange, partial image groups) is not in the kernel at all.  Exactly one
// such configuration exists per kernel: the world-1 step at 64 images per GPU with the
// default slicing (fwd: 3 pooled positions per slice, 16 images per block; bwd: 2 positions,
// single chunk), eager W1 update.  The last slice of either grid is shorter than PP
// (NPOS = 169 = 56 * 3 + 1 = 84 * 2 + 1): it runs the same constant-trip code with the
// operands of positions >= NPOS staged as zeros (0 x finite leaves the fp32 MFMA / fmaf sums
// unchanged bit for bit) and their global loads, stores and atomics predicated off.
//
// How the forward spreads its phases over the block's waves (fwd only; every choice moves
// whole tiles or stores between waves, none changes a value or an order of additions):
//   NT      threads per block (NT / 64 waves)
//   BAL     conv + pool row tiles: 0 round-robin over the waves (the flagship's 12 tiles on 8
//           waves: four waves build two tiles, four build one), 1 as 0 with NT = 768 (12 waves,
//           one tile each), 2 the leftover tiles split by channel half (8 waves: one tile
//           plus one half tile each)
//   STORES  the pooled tile / argmax codes go to global memory 0 before dense-1 (all
//           threads), 1 by the waves without a dense-1 tile while the others run it, 2 by all
//           threads after the dense-1 atomics
//   D1REG   the dense-1 waves add their accumulators to hacc straight from registers (4
//           atomic instructions per wave, four 128-B row segments each) instead of LDS store,
//           barrier, one 512-B row per instruction
// The generic kernels keep 0 / 0 / 0 on 512 threads: the bitwise comparison of the two
// instantiations (tests/test_convnet_specialised_gpu.py, test_convnet_fwd_balance_gpu.py) is
// the check of the flagship's.  The DAMD_FWD_* macros exist for A/B builds of the variants.
// Measured (BENCH.md, round 8): 1 / 1 / 1 is the fastest.  The conv phase itself does not gain
// from BAL -- its 12 tiles are 3 per SIMD whatever the wave count, and the SIMD's VALU issue
// is the limit (the waves that share a SIMD with an older one arrive last) -- but with 12
// waves the prologue is shorter (one W1 unit per thread) and eight waves, not four, move the
// stores while four run dense-1; BAL = 2 (a duplicated A-fragment build) loses.  Re-checked in
// round 10, after the conv phase lost its lane-constant setup: BAL = 0 is still slower than 1.
#ifndef DAMD_FWD_BAL
#define DAMD_FWD_BAL 1
#endif
#ifndef DAMD_FWD_STORES
#define DAMD_FWD_STORES 1
#endif
#ifndef DAMD_FWD_D1REG
#define DAMD_FWD_D1REG 1
#endif
//
// How the backward spreads its phases over the block's waves (bwd only; as above, every choice
// moves whole tiles, taps or stores between waves, none changes a value or an order of additions):
//   NT      threads per block, 512 or 1024.  1024 (16 waves): h 4 columns per thread; logits /
//           softmax on waves 0-3 as before; the body staged by waves 4-15 (pooled tile and input
//           rows one slot per thread on waves 4-11, argmax codes and the W1 slice on waves
//           12-15); dh, dW1 (+ eager update) and dP one 16x16 tile per wave; the conv gradient
//           split by taps (threads 0-511 taps 0-4, threads 512-1023 taps 5-8 and the bias sum,
//           each chain in its (image, position) order from zero)
//   AUX     0 the block's aux sums and a barrier sit between dh and the dW1 MFMAs, because dps
//           aliases the head scratch; 1 dps has its own LDS region, the barrier is gone and the
//           aux sums run behind the dP MFMAs
// The generic kernels keep 512 / 0.  The DAMD_BWD_* macros exist for A/B builds of the variants.
// Measured (BENCH.md, round 9): 1024 / 1 is the fastest.  Issuing the zeroing of the dead hacc
// parity and the next step's rows early, by the waves without a logits tile, loses at either
// wave count; the aux sums in the tail measure the same as behind the MFMAs.
#ifndef DAMD_BWD_NT
#define DAMD_BWD_NT 1024
#endif
#ifndef DAMD_BWD_AUX
#define DAMD_BWD_AUX 1
#endif
//   SPLIT   0 one block per slice runs the head and then both groups of work behind dh, one
//           after the other; 1 a grid of 2 NS blocks, a role per block (block-uniform, scalar):
//           blocks 0 .. NS - 1 the conv role of slice blockIdx.x, blocks NS .. 2 NS - 1 the W1
//           role of slice blockIdx.x - NS.  Both run the head as before.
//             conv role  stages the bf16 W1 slice, the argmax codes and the input rows; builds
//                        only dhs (the A-operand layout of dh); dP MFMAs, the conv gradient, the
//                        `red` hand-off (a region of its own: no barrier ahead of it) and the
//                        hconv atomics.  The kernel's critical chain.
//             W1 role    stages the pooled tile and the slice's fp32 masters / velocities; builds
//                        only dht; dW1 MFMAs, the eager update and its stores; then everything
//                        that sits off the chain: the aux sums and their b1 / W2 / b2 gradient and
//                        metric-tail stores, the zeroing of the dead hacc parity, the next-batch
//                        rows and their tag.
//           Neither role executes the other's code or loads / stages its operands; block 0 alone
//           advances the ctrl block.  The mapping of aux elements, zeroing ranges and next-batch
//           units by slice is the unsplit kernel's, so every thread forms the same sums.
//           The two blocks of a slice are not ordered: the conv role reads the bf16 W1 slice the
//           W1 role rewrites, which is why the bf16 copy has one buffer per step parity (below).
//           Measured (BENCH.md, round 11): 1 is the faster -- the conv role's chain ends 0.6 us
//           earlier, the kernel 0.4 us.
#ifndef DAMD_BWD_SPLIT
#define DAMD_BWD_SPLIT 1
#endif
//   FIXW    the fixed-point decodes of the flagship kernels (bwd: the four dense-1 sums a thread
//           turns into h; fwd: the pending conv gradient): 0 from_fix, 1 from_fix_wave -- the
//           narrow form when a wave-uniform test finds every value inside it, from_fix otherwise
//   CGPRE   the conv gradient: 0 conv_grad, which decodes each argmax code where it uses it; 1 the
//           staging waves translate the codes into pre-decoded entries (code_entries) and the
//           gradient reads entries, dP values and x taps in two LDS batches, addresses from
//           per-thread bases and immediate offsets.  Same products, same order of additions.
// The generic kernels keep 0 / 0: flagship against generic compares the new code with the old.
#ifndef DAMD_FIXW
#define DAMD_FIXW 1
#endif
#ifndef DAMD_BWD_CGPRE
#define DAMD_BWD_CGPRE 1
#endif
// The bf16 copy of W1 is double-buffered by step parity: in a step of parity p every reader
// (fwd's dense-1 operand, bwd's dP operand) reads buffer p, and the eager update in bwd writes
// buffer p ^ 1, which the next step (parity p ^ 1) reads; the deferred update in fwd writes
// buffer p, which the same step's bwd reads.  flush leaves parity 0: it writes buffer 0
// (deferred) or, eager, w1bf_live0 copies buffer 1 over buffer 0 first when the parity was 1.
// No reader and writer of one launch share a buffer, so nothing depends on how blocks are
// placed or ordered.  The kernels receive the pair as (live, other) when the host knows the
// parity (par_hint >= 0) and as (buffer 0, buffer 1) when it does not; then they pick by the
// ctrl block's parity and load the slice behind the ctrl block.
struct CfgGeneric {
  static constexpr int PP = 0, LG = 0;
  static constexpr bool B64 = false, EAGER = false, SH = true;  // SH: may be sharded (xa.world)
  static constexpr int NT = 512, BAL = 0, STORES = 0;
  static constexpr bool D1REG = false;
  static constexpr int AUX = 0, SPLIT = 0;
  static constexpr bool FIXW = false, CGPRE = false;
};
struct CfgFlagFwd {
  static constexpr int PP = 3, LG = 4;
  static constexpr bool B64 = true, EAGER = true, SH = false;
  static constexpr int BAL = DAMD_FWD_BAL, STORES = DAMD_FWD_STORES, NT = BAL == 1 ? 768 : 512;
  static constexpr bool D1REG = DAMD_FWD_D1REG != 0, FIXW = DAMD_FIXW != 0;
  static_assert(BAL >= 0 && BAL <= 2 && STORES >= 0 && STORES <= 2, "fwd wave mapping");
};
struct CfgFlagBwd {
  static constexpr int PP = 2, LG = 0;
  static constexpr bool B64 = true, EAGER = true, SH = false;
  static constexpr int NT = DAMD_BWD_NT, AUX = DAMD_BWD_AUX, SPLIT = DAMD_BWD_SPLIT;
  static constexpr bool FIXW = DAMD_FIXW != 0, CGPRE = DAMD_BWD_CGPRE != 0 && NT == 1024;  // (CGPRE builds on 16 waves)
  static_assert((NT == 512 || NT == 1024) && AUX >= 0 && AUX <= 1 && SPLIT >= 0 && SPLIT <= 1, "bwd wave mapping");
  // blocks of the grid
  static constexpr int NSC = (convnet::NPOS + PP - 1) / PP, GRID = SPLIT ? 2 * NSC : NSC;
};
// aux elements (b1/W2/b2 gradients + metric tail) per bwd block, and a power-of-two thread
// count per element (<= 64) that fits them in 512 threads: chunk_aux | log2(threads) << 16
__host__ __device__ constexpr int aux_split(int NS) {
  const int chunk_aux = (NAUX2 + NS - 1) / NS;
  int ltpe = 0;
  while (ltpe < 6 && (2 << ltpe) * chunk_aux <= 512) ++ltpe;
  return chunk_aux | (ltpe << 16);
}

// =================================================================================
// fwd: grid (NS slices, IG image groups of IB = 2^lg images)
// =================================================================================
template <bool U8, class C>
// (the body of both fwd kernels below: fwd, every size a runtime value, and fwd_flag, the
// flagship configuration's constants folded -- bpp, lge and xa are not read there)
__device__ __forceinline__ void fwd_body(const void* __restrict__ xnext, uint16_t* __restrict__ w1bf,
                                         float* __restrict__ P, float* __restrict__ V,
                                         float* __restrict__ calt, const long long* __restrict__ hconv_r,
                                         const float* __restrict__ G, int bpp, int lge, Ctrl* __restrict__ ctrl,
                                         const void* __restrict__ X, float* __restrict__ W1alt,
                                         float* __restrict__ V1alt, uint16_t* __restrict__ pooled,
                                         uint8_t* __restrict__ code, long long* __restrict__ hacc,
                                         long long* __restrict__ hconv, unsigned long long* st, const XArgs& xa,
                                         const long long* __restrict__ xtag, const int* __restrict__ labels,
                                         void* __restrict__ xcur, int* __restrict__ ycur, int phint,
                                         uint16_t* __restrict__ w1bf_alt) {
  constexpr bool SPEC = C::PP > 0;
  static_assert(!SPEC || (C::B64 && C::EAGER && !C::SH && C::LG == 4), "the one constant configuration");
  // threads / waves of the block, 16-byte units of the bf16 W1 slice per thread (eager)
  constexpr int NT = C::NT, NW = NT / 64, NBQ = SPEC ? (C::PP * 32 * HID / 8 + NT - 1) / NT : 2;
  static_assert(NT % 64 == 0 && NT >= 512 && (SPEC || NT == 512), "row staging and the deferred update map 512 threads");
  static_assert(SPEC || (C::BAL == 0 && C::STORES == 0 && !C::D1REG), "the generic kernels keep the plain mapping");
  const int B = SPEC ? CH : bpp & 0xffff, PP = SPEC ? C::PP : bpp >> 16, lg = SPEC ? C::LG : lge & 0xff;
  const int eager = SPEC ? 1 : lge >> 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // (wave through readfirstlane: the compiler then knows it is uniform, so a tile's coordinates
  // are scalar work and the role branches -- wave < ntiles -- scalar branches)
  const int s = blockIdx.x, tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const bool sh = C::SH && xa.world > 1;  // sharded multi-rank step: gradients from the exchange staging
  constexpr int hprobe = DAMD_PROBE_HACC;  // 0 in every product build (see the top of the file)
  // (constant configuration: the grid is NS x B / IB blocks, every image group is full)
  constexpr int NSC = SPEC ? (NPOS + C::PP - 1) / C::PP : 0, IGC = SPEC ? CH >> C::LG : 0;
  const int gx = SPEC ? NSC : (int)gridDim.x;
  const int nblk = SPEC ? NSC * IGC : (int)(gridDim.x * gridDim.y), lin = blockIdx.y * gx + s;
  Stamps sts;
  stamp(sts, st, 0);
  const int IB = 1 << lg, img0 = blockIdx.y * IB;
  const int BP = (B + CH - 1) / CH * CH;
  const int p0 = s * PP, p1 = min(NPOS, p0 + PP), np = p1 - p0, K = np * 32;
  const int KP = kpitch(PP);
  // trip count of the slice loops, pitch of the argmax-code tile: the constant PP, not np
  const int npl = SPEC ? PP : np, KC = npl * 32;
  float* xs = reinterpret_cast<float*>(smem);                              // [IB][XR][28]; later [IB][64] partials
  uint16_t* as = reinterpret_cast<uint16_t*>(smem + IB * XR * IMG * 4);    // [IB][KP] pooled tile
  uint16_t* w1t = as + IB * KP;                                            // [HID][KP] W1 slice^T
  uint16_t* wf = w1t + HID * KP;                                           // [2][64][8] conv weight fragments
  float* cb = reinterpret_cast<float*>(wf + WF_BYTES / 2);                 // [32] conv biases
  static_assert(NT >= NCONV + 5 * NF, "threads past the conv parameters zero the pad slots");
  const int n4 = K * HID / 4;  // <= 2048
  const int r0 = 2 * (p0 / PO);
  const int nrows = 2 * ((p1 - 1) / PO) + 4 - r0;
  // ---- the batch rows as the previous step's bwd prefetched them (xnext): issued first,
  // before the ctrl block is known; kept below if their tag names this step's rows ----
  XStage<U8> xst;
  long long xt = 0;
  // (the row-staging map covers 512 threads: the waves past them take the idle slot -1)
  const int xslot = NT > 512 && tid >= 512 ? -1 : tid;
  if (xnext != nullptr) {
    x_load<U8>(xst, xnext, img0, B, SPEC ? IB : B - img0, lg, r0, nrows, xslot);
    xt = *xtag;
  }
  // ---- first the loads whose addresses do not depend on the ctrl block: the bf16 W1 slice
  // (eager), both parities of the conv parameters, the b1/W2/b2 triplet; the scheduling
  // barrier keeps them ahead of the ctrl load (left alone, hipcc issued the ctrl load first
  // and waited for it with the kernel arguments, then sank these below further waits) ----
  uint4 bq[NBQ];  // eager: the bf16 W1 slice (bwd already applied the update)
  // (the bf16 copy has one buffer per step parity: this step reads and -- deferred update --
  // writes the live one.  Known parity: the host passed the live buffer as w1bf; else w1bf /
  // w1bf_alt are buffers 0 / 1 and the load waits for the ctrl block's parity)
  auto load_bq = [&](const uint16_t* __restrict__ src) __attribute__((always_inline)) {
    // (lanes past the slice load nothing: at PP = 2 the second unit is all out of range, and
    // its clamped duplicate loads were 8 KB per block of wasted load bandwidth.  Written as a
    // conditional load, not a select between pointers: hipcc turns the latter into a flat
    // load from a zero vector in scratch)
#pragma unroll
    for (int u = 0; u < NBQ; ++u) {
      bq[u] = make_uint4(0u, 0u, 0u, 0u);
      if (tid + u * NT < n4 / 2) bq[u] = reinterpret_cast<const uint4*>(src + p0 * 32 * HID)[tid + u * NT];
    }
  };
  if (eager && phint >= 0) load_bq(w1bf);
  // conv parameters: current buffer by parity; their gradient is the previous step's
  // (bwd added it into hconv[par ^ 1])
  const int tcl = min(tid, NCONV - 1);
  const float cp0 = P[tcl], cp1 = calt[tcl], cv0 = V[tcl], cv1 = calt[NCONV + tcl];
  const long long cq0 = sh ? 0 : hconv_r[NCONV + tcl], cq1 = sh ? 0 : hconv_r[tcl];
  // b1/W2/b2: the grid's last two blocks own their pending update (nobody else in this
  // launch reads them; bwd reads the updated values)
  const int si = (lin - (nblk - 2)) * NT + tid;
  const bool small_on = lin >= nblk - 2 && si >= 0 && si < NSMALL;
  const int sic = OFF_B1 + max(0, min(si, NSMALL - 1));
  const float sp = P[sic], sg0 = sh ? 0.f : G[sic], sv = V[sic];
  // where this thread's conv weight goes in the LDS fragment table: address math while the
  // loads above are in flight, not behind the wait for them
  int wfs[3];
  conv_w_slots(wfs, tid);
  __builtin_amdgcn_sched_barrier(0);

  const Ctrl c = *ctrl;
  const int par = phint >= 0 ? phint : c.wpar;
  if (phint >= 0 && phint != c.wpar && lin == 0 && tid == 0)
    __hip_atomic_fetch_or(&ctrl->bad, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned xe = (unsigned)c.xcnt;  // sharded: exchange epoch of the pending update
  if (lin == 0 && tid == 0) {
    ctrl->cur2 = c.cursor;
    ctrl->par2 = par;
    ctrl->xcnt2 = c.xcnt;
    ctrl->pend2 = c.pending;
  }
  const bool pend = c.pending != 0;
  const long row_base = (long)c.cursor * c.global_batch + c.row0 + img0;
  const bool mom = c.momentum != 0.f;
  uint16_t* w1live = phint < 0 && par ? w1bf_alt : w1bf;  // the bf16 W1 buffer of this step's parity
  if (eager && phint < 0) load_bq(w1live);

  // ---- then the ctrl-dependent loads: the batch rows unless prefetched (and, deferred
  // update, W1 by parity) ----
  const bool xhit = xnext != nullptr && xt == (((long long)c.xgen << 32) | (long long)(unsigned)(c.cursor + 1));
  if (!xhit) x_load<U8>(xst, X, row_base, c.nsamples, SPEC ? IB : B - img0, lg, r0, nrows, xslot);
  // this step's rows and labels for the backward (xcur / ycur): a share per block, from the
  // prefetch when it hit (L2-hot), else from the dataset; stored at the end of the kernel
  constexpr int UPI = U8 ? NPIX / 16 : NPIX / 4;  // 16-byte units per image
  const int xcu = lin * NT + tid;
  const bool xcp = xcur != nullptr && xcu < B * UPI;
  uint4 xcv = make_uint4(0u, 0u, 0u, 0u);
  int ycv = -1;
  {
    const long rb0 = (long)c.cursor * c.global_batch + c.row0;
    if (xcp) {
      const int b = xcu / UPI, q = xcu - b * UPI;
      if (xhit) xcv = reinterpret_cast<const uint4*>(xnext)[xcu];
      else if (rb0 + b < c.nsamples)
        xcv = reinterpret_cast<const uint4*>(static_cast<const char*>(X) +
                                             __umul24((unsigned)(rb0 + b), U8 ? NPIX : 4 * NPIX))[q];
    }
    if (xcur != nullptr && lin == 0 && tid < B && rb0 + tid < c.nsamples) ycv = labels[rb0 + tid];
  }
  float4 wv[4], gv[4], vv[4];
  const float* Wcur = par ? W1alt : P + OFF_W1;
  const float* Vcur = par ? V1alt : V + OFF_W1;
  float* Wnext = par ? P + OFF_W1 : W1alt;
  float* Vnext = par ? V + OFF_W1 : V1alt;
  const float4* P4 = reinterpret_cast<const float4*>(Wcur + p0 * 32 * HID);
  const float4* G4 = reinterpret_cast<const float4*>(G + OFF_W1 + p0 * 32 * HID);
  const float4* V4 = reinterpret_cast<const float4*>((mom ? Vcur : Wcur) + p0 * 32 * HID);
  const bool owner = blockIdx.y == 0;
  float4* Wn4 = reinterpret_cast<float4*>(Wnext + p0 * 32 * HID);
  float4* Vn4 = reinterpret_cast<float4*>(Vnext + p0 * 32 * HID);
  uint2* Wb = reinterpret_cast<uint2*>(w1live + p0 * 32 * HID);
  if (!eager) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ic = min(tid + u * 512, n4 - 1);
      wv[u] = P4[ic];
      gv[u] = sh ? make_float4(0.f, 0.f, 0.f, 0.f) : G4[ic];  // sharded: after its unit flags
      vv[u] = V4[ic];
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  const float cp = par ? cp1 : cp0, cv = par ? cv1 : cv0;
  long long cq = par ? cq1 : cq0;
  float sg = sg0;
  // sharded: the previous step's conv / b1 / W2 / b2 gradients and metric tail are the
  // rank-ordered sums of every rank's small message (published by each rank's last bwd block)
  if (sh && pend) {
    const int ps = xe & 1;
    float* xo = xa.out[xa.rank];
    if (tid < xa.world) x_wait(xa, x_sflag(xo, 4 * ((NPOS + xa.ppb - 1) / xa.ppb), ps, tid), xe, XW_SMALL);
    __syncthreads();
    long long q = 0;
    float g = 0.f;
    for (int r = 0; r < xa.world; ++r) {
      const float* m = x_small(xo, ps, r);
      q += reinterpret_cast<const long long*>(m + SM_CONV)[tcl];
      if (small_on) g += m[SM_GRAD + max(0, min(si, NSMALL - 1))];
    }
    cq = q;
    sg = g;
    if (lin == nblk - 1 && tid < 3) {  // fold the reduced metric tail into the epoch totals
      float a = 0.f;
      for (int r = 0; r < xa.world; ++r) a += x_small(xo, ps, r)[SM_MET + tid];
      float* accp = tid == 0 ? &ctrl->acc_loss : (tid == 1 ? &ctrl->acc_correct : &ctrl->acc_count);
      *accp = (tid == 0 ? c.acc_loss : (tid == 1 ? c.acc_correct : c.acc_count)) + a;
    }
  }

  // ---- pending SGD updates ----
  if (eager) {
#pragma unroll
    for (int u = 0; u < NBQ; ++u) {
      const int i = tid + u * NT;  // 8 consecutive n of row kr
      // (constant configuration: every row of the tile is written -- the short last slice's
      // rows past K with the zeros bq holds there, the dense-1 MFMAs run over all PP positions)
      if (i < (SPEC ? PP * 32 * HID / 8 : n4 / 2)) {
        const int e = i * 8, kr = e >> 6, n = e & 63;
        const uint32_t w[4] = {bq[u].x, bq[u].y, bq[u].z, bq[u].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          w1t[(n + 2 * q) * KP + kr] = (uint16_t)(w[q] & 0xffffu);
          w1t[(n + 2 * q + 1) * KP + kr] = (uint16_t)(w[q] >> 16);
        }
      }
    }
  }
  // deferred W1 update of the slice (registers -> bf16 W1^T tile in LDS; the image group 0
  // block also writes the next fp32 buffer, velocity and bf16 copy)
  auto w1_update = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = tid + u * 512;
      if (!eager && i < n4) {
        float4 wn, vn;
        sgd_or_keep(pend, wv[u].x, gv[u].x, vv[u].x, c, wn.x, vn.x);
        sgd_or_keep(pend, wv[u].y, gv[u].y, vv[u].y, c, wn.y, vn.y);
        sgd_or_keep(pend, wv[u].z, gv[u].z, vv[u].z, c, wn.z, vn.z);
        sgd_or_keep(pend, wv[u].w, gv[u].w, vv[u].w, c, wn.w, vn.w);
        const int e = i * 4, kr = e >> 6, n = e & 63;
        const uint16_t h0 = f2bf(wn.x), h1 = f2bf(wn.y), h2 = f2bf(wn.z), h3 = f2bf(wn.w);
        w1t[(n + 0) * KP + kr] = h0;
        w1t[(n + 1) * KP + kr] = h1;
        w1t[(n + 2) * KP + kr] = h2;
        w1t[(n + 3) * KP + kr] = h3;
        if (owner) {
          Wn4[i] = wn;
          if (mom) Vn4[i] = vn;
          Wb[i] = make_uint2((uint32_t)h0 | ((uint32_t)h1 << 16), (uint32_t)h2 | ((uint32_t)h3 << 16));
        }
      }
    }
  };
  if (!sh) w1_update();
  float cwn = 0.f, cvn = 0.f;
  if (tid < NCONV) {  // (5 whole waves)
    float cg[1];
    const long long cqa[1] = {cq};
    if constexpr (C::FIXW) from_fix_wave(cg, cqa, CINV);
    else cg[0] = from_fix(cq, CINV);
    sgd_or_keep(pend, cp, cg[0], cv, c, cwn, cvn);
    // weights: split once here and stored in MFMA operand order, not per wave and lane
    if (tid < OFF_BC) conv_w_store(wf, wfs, cwn);
    else cb[tid - OFF_BC] = cwn;
    // the conv epilogue's ReLU (fmaxf) and the head's would turn a NaN parameter into 0:
    // a non-finite conv / b1 / W2 / b2 value raises ctrl.bad (loss NaN) here instead
    if (!__builtin_isfinite(cwn)) __hip_atomic_fetch_or(&ctrl->bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (tid >= NCONV && tid < NCONV + 5 * NF) wf[wfs[0]] = 0;
  if (small_on) {
    float wn, vn;
    sgd_or_keep(pend, sp, sg, sv, c, wn, vn);
    P[sic] = wn;
    if (mom) V[sic] = vn;
    if (!__builtin_isfinite(wn)) __hip_atomic_fetch_or(&ctrl->bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the owner writes the next conv buffer and zeroes the hconv parity bwd adds into next
  if (lin == 0 && tid < NCONV) {
    (par ? P : calt)[tid] = cwn;
    if (mom) (par ? V : calt + NCONV)[tid] = cvn;
    hconv[par * NCONV + tid] = 0;
  }
  stamp(sts, st, 1);
  x_store<U8>(xst, xs, lg, nrows);
  lds_barrier();
  stamp(sts, st, 2);

  ConvFrag cf;
  conv_setup(cf, wf, cb, lane);
  stamp(sts, st, 5);
  uint8_t* csl = reinterpret_cast<uint8_t*>(cb + NF);  // [IB][KC] argmax codes
  // (image bu + bl: bu and plo are wave-uniform, so the tile's store base is scalar work)
  conv_pool<NW, C::BAL == 2>(cf, xs, p0, npl, r0, lg, wave, lane, [&](int bu, int bl, int plo, int ch, uint16_t hb, uint8_t cd) {
    // (constant configuration: positions >= NPOS of the last slice were computed from rows
    // nobody staged; their pooled value is 0, their code is never stored)
    as[(bu * KP + plo * 32) + (bl * KP + ch)] = SPEC && plo >= np ? (uint16_t)0 : hb;
    csl[(bu * KC + plo * 32) + (bl * KC + ch)] = cd;
  });
  stamp(sts, st, 6);
  lds_barrier();
  stamp(sts, st, 3);
  // pooled tile (feature-major [k][b]: bwd's dW1 operand) and argmax codes ([b][k]) for
  // bwd, from LDS as contiguous 8-byte / 4-byte stores instead of scattered 1-2 B stores
  // (IB / 4 = 2^(lg - 2) and K / 4 = 8 np: shifts and a multiply, not divisions)
  // t0 / nt: the calling thread's slot among the nt threads that share the stores (dense-1
  // reads only the LDS copies, so where these stores sit is a scheduling choice: C::STORES)
  auto store_out = [&](int t0, int nt) __attribute__((always_inline)) {
    for (int i = t0; i < KC * (IB / 4); i += nt) {
      if (SPEC && i >= K * (IB / 4)) break;
      const int kk = i >> (lg - 2), bo = 4 * (i & ((1 << (lg - 2)) - 1));
      uint16_t v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = as[(bo + e) * KP + kk];
      uint16_t* dst = pooled + (unsigned)((p0 * NF + kk) * BP + img0 + bo);
      if (SPEC || img0 + bo + 3 < B) {
        *reinterpret_cast<uint2*>(dst) = make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16),
                                                   (uint32_t)v[2] | ((uint32_t)v[3] << 16));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (img0 + bo + e < B) dst[e] = v[e];
      }
    }
    for (int i = t0; i < IB * (KC / 4); i += nt) {
      const int i8 = i >> 3, bo = npl == 3 ? (int)(((unsigned)i8 * 21846u) >> 16) : i8 >> (npl >> 1), w = i - bo * (KC / 4);
      if ((SPEC || img0 + bo < B) && (!SPEC || 4 * w < K))
        *reinterpret_cast<uint32_t*>(code + (unsigned)((img0 + bo) * FEAT + p0 * NF + 4 * w)) =
            reinterpret_cast<const uint32_t*>(csl + bo * KC)[w];
    }
    stamp(sts, st, 7);
  };
  if (C::STORES == 0) store_out(tid, NT);
  if (sh) {
    // sharded: the slice's reduced dW1 arrives as 4 units (2 halves each) from their owners,
    // pushed at the end of every owner's bwd -- waited for only now, after the conv
    if (pend) {
      // units of the bwd slices covering this slice's rows, 2 halves each
      const int sb0 = p0 / xa.ppb, nunits = 4 * ((p1 - 1) / xa.ppb - sb0 + 1), NUb = 4 * ((NPOS + xa.ppb - 1) / xa.ppb);
      if (tid < 2 * nunits) x_wait(xa, x_gflag(xa.out[xa.rank], NUb, 4 * sb0 + (tid >> 1), tid & 1), xe, XW_UNIT);
      __syncthreads();
      if (xa.gbf16) {
        const uint2* R2 = reinterpret_cast<const uint2*>(xa.out[xa.rank] + kXG16) + p0 * 32 * HID / 4;
#pragma unroll
        for (int u = 0; u < 4; ++u) gv[u] = unpack_bf16x4(R2[min(tid + u * 512, n4 - 1)]);
      } else {
        const float4* R4 = reinterpret_cast<const float4*>(xa.out[xa.rank] + kXGred + OFF_W1 + p0 * 32 * HID);
#pragma unroll
        for (int u = 0; u < 4; ++u) gv[u] = R4[min(tid + u * 512, n4 - 1)];
      }
    }
    w1_update();
    lds_barrier();
  }
  // ---- dense-1 partial of the slice: part[row][n] = sum_k pooled[row][k] W1[k][n] ----
  const int ko = 8 * (lane >> 4);
  const int ntiles = (IB >> 4) * 4;
  float* part = xs;  // [IB][64] (the staged rows are dead)
  long long* hp = hacc + (long)par * B * HACC_PITCH;
  // the threads of the waves without a dense-1 tile (C::STORES == 1: they store the pooled
  // tile and the codes meanwhile)
  const int TD1 = ntiles * 64;
  static_assert(!(C::D1REG || C::STORES == 1) || ((1 << C::LG) >> 4) * 4 < NW, "dense-1 tiles: one per wave, waves to spare");
  if constexpr (C::D1REG) {
    // one tile per wave, added to hacc from the accumulator registers: lane (q, n) holds rows
    // 4 q .. 4 q + 3 of column n, so instruction j adds row 4 q + j of four rows' 128-B
    // segments -- no LDS round trip, no barrier ahead of the atomics (the values are the
    // ones the LDS path converts: part[] holds the accumulators unchanged)
    if (wave < ntiles) {
      const int mt = wave >> 2, nt = wave & 3;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const int ar = 16 * mt + (lane & 15), bn = 16 * nt + (lane & 15);
      for (int ks = 0; ks < npl; ++ks) {
        const bf16x8 a = ld_frag(as + ar * KP + ks * 32 + ko);
        const bf16x8 bb = ld_frag(w1t + bn * KP + ks * 32 + ko);
        acc = mfma16(a, bb, acc);
      }
      stamp(sts, st, 8);
#pragma unroll
      for (int j = 0; j < (hprobe == 1 ? 0 : hprobe == 2 ? 2 : 4); ++j) {
        const int r = 16 * mt + 4 * (lane >> 4) + j;
        atomic_add_i64(hp + (unsigned)((img0 + r) * HACC_PITCH + bn), to_fix(acc[j], HSCALE, &ctrl->bad));
      }
    } else {
      if (C::STORES == 1) store_out(tid - TD1, NT - TD1);
      stamp(sts, st, 8);
    }
    stamp(sts, st, 9);  // (no dense-1 barrier: the slot repeats the one before)
  } else {
    for (int t = wave; t < ntiles; t += NW) {
      const int mt = t >> 2, nt = t & 3;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const int ar = 16 * mt + (lane & 15), bn = 16 * nt + (lane & 15);
      for (int ks = 0; ks < npl; ++ks) {
        const bf16x8 a = ld_frag(as + ar * KP + ks * 32 + ko);
        const bf16x8 bb = ld_frag(w1t + bn * KP + ks * 32 + ko);
        acc = mfma16(a, bb, acc);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) part[(16 * mt + 4 * (lane >> 4) + j) * HID + bn] = acc[j];
    }
    if (C::STORES == 1 && wave >= ntiles) store_out(tid - TD1, NT - TD1);
    stamp(sts, st, 8);
    lds_barrier();
    stamp(sts, st, 9);
    // one wave instruction = one 512-B row of 64 int64 adds
    for (int r = wave; r < (hprobe == 1 ? 0 : hprobe == 2 ? IB / 2 : IB); r += NW)
      if (SPEC || img0 + r < B) atomic_add_i64(hp + (unsigned)((img0 + r) * HACC_PITCH + lane), to_fix(part[r * HID + lane], HSCALE, &ctrl->bad));
  }
  if (C::STORES == 2) store_out(tid, NT);
  if (xcp) reinterpret_cast<uint4*>(xcur)[xcu] = xcv;
  if (xcur != nullptr && lin == 0 && tid < B) ycur[tid] = ycv;
  stamp(sts, st, 4);
  if (st != nullptr && lin < 256) {
    if (tid == 0)
      for (int i = 0; i < 10; ++i) st[lin * 16 + i] = C::STORES == 1 && i == 7 ? 0ull : sts.t[i];  // (7: not wave 0's)
    // the stamps above are wave 0's.  Slots 10-13: the view of one other wave per block
    // (block lin: wave lin mod NW, so the grid covers every wave ~nblk / NW times) of conv
    // setup, conv pool (its arrival at the post-conv barrier), dense-1 mfma (its arrival at
    // the dense-1 barrier) and atomics issued; slot 14: that wave | waves per block << 8
    const int wsel = lin % NW;
    if (tid == 64 * wsel) {
      st[lin * 16 + 10] = sts.t[5];
      st[lin * 16 + 11] = sts.t[6];
      st[lin * 16 + 12] = sts.t[8];
      st[lin * 16 + 13] = sts.t[4];
      st[lin * 16 + 14] = (unsigned long long)(wsel | (NW << 8));
    }
  }
}

template <bool U8>
// (ctrl and X lead the argument list: with kernarg preloading they arrive in SGPRs, so
// the first dependent loads -- the ctrl block, then the batch rows -- start at once)
// (the first 16 argument dwords arrive preloaded in SGPRs: the pointers of the prologue's
// first loads and the packed sizes their addresses need -- bpp = B | PP << 16, lge = lg |
// eager << 8; later arguments come from the kernarg segment, a scalar load's latency behind)
__global__ __launch_bounds__(512) void fwd(const void* __restrict__ xnext, uint16_t* __restrict__ w1bf,
                                           float* __restrict__ P, float* __restrict__ V,
                                           float* __restrict__ calt, const long long* __restrict__ hconv_r,
                                           const float* __restrict__ G, int bpp, int lge, Ctrl* __restrict__ ctrl,
                                           const void* __restrict__ X, float* __restrict__ W1alt,
                                           float* __restrict__ V1alt, uint16_t* __restrict__ pooled,
                                           uint8_t* __restrict__ code, long long* __restrict__ hacc,
                                           long long* __restrict__ hconv, unsigned long long* st, const XArgs xa,
                                           const long long* __restrict__ xtag, const int* __restrict__ labels,
                                           void* __restrict__ xcur, int* __restrict__ ycur, int phint,
                                           uint16_t* __restrict__ w1bf_alt) {
  fwd_body<U8, CfgGeneric>(xnext, w1bf, P, V, calt, hconv_r, G, bpp, lge, ctrl, X, W1alt, V1alt, pooled, code, hacc,
                           hconv, st, xa, xtag, labels, xcur, ycur, phint, w1bf_alt);
}

// The flagship configuration (CfgFlagFwd): no packed sizes, no exchange arguments, no W1
// double buffer (eager: fwd reads only the bf16 copy).  The preloaded 16 dwords are the
// pointers of the loads issued ahead of the ctrl block, the prefetch tag among them.
template <bool U8>
__global__ __launch_bounds__(CfgFlagFwd::NT) void fwd_flag(const void* __restrict__ xnext,
                                                const long long* __restrict__ xtag,
                                                uint16_t* __restrict__ w1bf, float* __restrict__ P,
                                                float* __restrict__ V, float* __restrict__ calt,
                                                const long long* __restrict__ hconv_r, const float* __restrict__ G,
                                                Ctrl* __restrict__ ctrl, const void* __restrict__ X,
                                                uint16_t* __restrict__ pooled, uint8_t* __restrict__ code,
                                                long long* __restrict__ hacc, long long* __restrict__ hconv,
                                                unsigned long long* st, const int* __restrict__ labels,
                                                void* __restrict__ xcur, int* __restrict__ ycur, int phint,
                                                uint16_t* __restrict__ w1bf_alt) {
  fwd_body<U8, CfgFlagFwd>(xnext, w1bf, P, V, calt, hconv_r, G, 0, 0, ctrl, X, nullptr, nullptr, pooled, code, hacc,
                           hconv, st, XArgs{}, xtag, labels, xcur, ycur, phint, w1bf_alt);
}

// =================================================================================
// sharded exchange, end of bwd (every wave of every block calls it)
// =================================================================================
//  1. the partial pushes of this wave have drained (nothing else was issued since, so the
//     wait costs nothing): raise the partial flag at the owner
//  2. arrival ticket: the last block of the launch reads this rank's conv-gradient int64
//     sums, b1 / W2 / b2 gradient and metric tail (all complete: every block drained its
//     stores before its ticket) and publishes them as this rank's small message on every rank
//  3. owner waves: wait for the other ranks' halves of their unit, sum the world partials
//     in rank order (own from registers), push the reduced unit to every rank's gradient
//     staging, raise the unit flag there
__device__ __forceinline__ void exchange_tail(const XArgs& xa, Ctrl* ctrl, const float* G, const long long* hconv_p,
                                              const f32x4* accw, unsigned xe, int s, int NS, int np, int p0, int dn,
                                              int dm0, int lane, int tid, bool xown, int xo, int xu) {
  __shared__ int last_flag;
  const int NU = 4 * NS, W = xa.world, ps = xe & 1;
  damd_publish_drain();
  DAMD_PUBLISH_WAVE();
  if (!xown && lane == 0) x_signal(x_pflag(xa.out[xo], xu, xa.rank * 2 + dm0), xe);
  // 2. ticket (counts forever: NS arrivals per step)
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const int t = __hip_atomic_fetch_add(&ctrl->ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = (t % NS) == NS - 1;
    if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    last_flag = last;
  }
  __syncthreads();
  if (last_flag) {
    const float* hc = reinterpret_cast<const float*>(hconv_p);
    for (int i = tid; i < SM_MET + 3; i += 512) {
      const float v = i < SM_GRAD ? hc[i] : (i < SM_MET ? G[OFF_B1 + i - SM_GRAD] : G[OFF_LOSS + i - SM_MET]);
      for (int r = 0; r < W; ++r) x_small(xa.out[r], ps, xa.rank)[i] = v;
    }
    // publish: EVERY wave drains its own small-message stores before the barrier (a
    // workgroup barrier does not wait for outstanding vector-memory stores), then the
    // flag -- the order scripts/check_publish_isa.py verifies on the gfx950 code object
    damd_publish_drain();
    __syncthreads();
    DAMD_PUBLISH_WG();
    if (tid < W) x_signal(x_sflag(xa.out[tid], NU, ps, xa.rank), xe);
  }
  // 3. owners
  if (xown) {
    if (lane < W && lane != xa.rank) x_wait(xa, x_pflag(xa.out[xa.rank], xu, lane * 2 + dm0), xe, XW_PART);
    asm volatile("" ::: "memory");
    f32x4 g[MAXPP];
#pragma unroll
    for (int i = 0; i < MAXPP; ++i) g[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < W; ++r) {
      const float* slot = xa.in[xa.rank] + ((long)r * NU + xu) * kXPSlot;
#pragma unroll
      for (int i = 0; i < MAXPP; ++i) {
        if (i >= np) break;
        float4 v;
        if (xa.gbf16)  // own partial rounded like the others': the sum is symmetric in the ranks
          v = unpack_bf16x4(r == xa.rank ? pack_bf16x4(accw[i])
                                         : reinterpret_cast<const uint2*>(slot)[(dm0 * MAXPP + i) * 64 + lane]);
        else
          v = r == xa.rank ? make_float4(accw[i][0], accw[i][1], accw[i][2], accw[i][3])
                           : reinterpret_cast<const float4*>(slot)[(dm0 * MAXPP + i) * 64 + lane];
        g[i][0] += v.x;
        g[i][1] += v.y;
        g[i][2] += v.z;
        g[i][3] += v.w;
      }
    }
    const int lr16 = lane & 15;
    if (xa.gbf16) {
      // bf16 reduced unit, row-major [k][n]: column pairs packed into 32-bit words (the even
      // lane of each pair stores both), i.e. 16 lanes write one 32-byte row piece
      for (int r = 0; r < W; ++r) {
        uint32_t* dst = reinterpret_cast<uint32_t*>(xa.out[r] + kXG16) + ((long)p0 * 32 * HID + 16 * dn + lr16) / 2;
#pragma unroll
        for (int i = 0; i < MAXPP; ++i) {
          if (i >= np) break;
          const int mt = dm0 + 2 * i;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t h = f2bf(g[i][j]);
            const uint32_t o = (uint32_t)__shfl_xor((int)h, 1);
            if (!(lr16 & 1)) dst[(16 * mt + 4 * (lane >> 4) + j) * (HID / 2)] = h | (o << 16);
          }
        }
      }
    } else {
      for (int r = 0; r < W; ++r) {
        float* dst = xa.out[r] + kXGred + OFF_W1 + (long)p0 * 32 * HID + 16 * dn + lr16;
#pragma unroll
        for (int i = 0; i < MAXPP; ++i) {
          if (i >= np) break;
          const int mt = dm0 + 2 * i;
#pragma unroll
          for (int j = 0; j < 4; ++j) dst[(16 * mt + 4 * (lane >> 4) + j) * HID] = g[i][j];
        }
      }
    }
    damd_publish_drain();
    DAMD_PUBLISH_WAVE();
    if (lane < W) x_signal(x_gflag(xa.out[lane], NU, xu, dm0), xe);
  }
}

// =================================================================================
// bwd: grid NS slices
// =================================================================================
// aux element e (parameter order at G + OFF_B1): [0,64) db1, [64,704) dW2
// (k = (e-64)/10, c = (e-64)%10), [704,714) db2, then 714 loss, 715 correct, 716 count.
template <bool U8, bool ONE, class C>  // ONE: B <= 64, a single chunk (no loop-carried prefetch registers)
// (the body of both bwd kernels below: bwd, every size a runtime value, and bwd_flag, the
// flagship configuration's constants folded -- bpp, eager_, xa and auxm_ are not read there)
__device__ __forceinline__ void bwd_body(long long* __restrict__ hacc, const int* __restrict__ ycur,
                                         const void* __restrict__ xcur, int phint, int bpp, const float* P,
                                         const uint16_t* w1bf, const uint16_t* __restrict__ pooled,
                                         const uint8_t* __restrict__ code, Ctrl* __restrict__ ctrl,
                                         const void* __restrict__ X, const int* __restrict__ labels,
                                         float* __restrict__ G, long long* __restrict__ hconv,
                                         int eager_, float* Pw, float* Vw, uint16_t* w1bf_out,
                                         unsigned long long* st, const float* __restrict__ Gr, const XArgs& xa,
                                         void* __restrict__ xnext, long long* __restrict__ xtag, int auxm_) {
  constexpr bool SPEC = C::PP > 0;
  static_assert(!SPEC || (ONE && C::B64 && C::EAGER && !C::SH), "the one constant configuration");
  const int B = SPEC ? CH : bpp & 0xffff, PP = SPEC ? C::PP : bpp >> 16;  // (packed: both preloaded)
  const int eager = SPEC ? 1 : eager_;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bool sh = C::SH && xa.world > 1;  // sharded multi-rank step (see the exchange at the end)
  constexpr int cprobe = DAMD_PROBE_HCONV;  // 0 in every product build (see the top of the file)
  Stamps sts;
  unsigned long long wst_dh = 0, wst_cg = 0;  // this wave's arrival at two barriers (slots 14 / 15)
  unsigned long long wst_red = 0;             // and at the barrier ahead of the `red` reduction (extra rows)
  stamp(sts, st, 0);
  constexpr int NSC = SPEC ? (NPOS + C::PP - 1) / C::PP : 1;  // (constant configuration: the slices)
  // a role per block (CfgFlagBwd::SPLIT; blockIdx.x is scalar, so every role branch is a scalar
  // branch): the conv role first -- blocks are dealt in index order and it is the critical one
  constexpr bool SPLIT = SPEC && C::SPLIT != 0;
  const int wrole = SPLIT && (int)blockIdx.x >= NSC ? 1 : 0;
  const bool rconv = !SPLIT || wrole == 0, rw1 = !SPLIT || wrole == 1;  // (unsplit: both, constants)
  const int s = SPLIT ? (int)blockIdx.x - wrole * NSC : (int)blockIdx.x, tid = threadIdx.x;
  const int NS = SPEC ? NSC : (int)gridDim.x;
  const bool blk0 = blockIdx.x == 0;  // the one block that advances the ctrl block
  const int auxm = SPEC ? aux_split(NSC) : auxm_;
  const int p0 = s * PP, p1 = min(NPOS, p0 + PP), np = p1 - p0, K = np * 32;
  const int KD = PP * 32 + 4;   // dps pitch (f32)
  const int KC = PP * 32;       // code pitch (bytes)
  // trip count of the slice loops: the constant PP, not np (short last slice: zero operands,
  // global loads / stores predicated off)
  const int npl = SPEC ? PP : np;
  // threads / waves of the block; W16: the 16-wave mapping (see CfgFlagBwd)
  constexpr int NT = C::NT, NW = NT / 64;
  constexpr bool W16 = NT == 1024, AUXD = C::AUX != 0;
  static_assert(SPEC || (NT == 512 && !AUXD), "the generic kernels keep the plain mapping");
  // CGP: the code tile holds the conv gradient's pre-decoded entries (CfgFlagBwd::CGPRE), two bytes per code
  constexpr bool CGP = SPEC && C::CGPRE;
  static_assert(!CGP || W16, "the pre-decoded conv gradient builds on the 16-wave mapping");
  const int CSB = CH * KC * (CGP ? CGE_BYTES : 1);
  // (AUXD: dps behind the head scratch in a region of its own, so the head scratch stays
  // readable to the end of the kernel; convnet2_bwd_lds sizes the flagship's LDS for it)
  const int RB = AUXD ? HEAD_BYTES + CH * KD * 4 : max(CH * KD * 4, HEAD_BYTES);
  // byte offsets of the LDS regions.  One block per slice: xs | head (dps behind it or aliasing
  // it) | pt | dht | dhs | w1s | cs, `red` over pt / dht and `ared` over dps once they are dead.
  // A role per block (convnet2_bwd_role_lds sizes the same layouts; the head leads both, so
  // every offset is a constant of the code that uses it, none a per-role select):
  //   conv role  head | xs | dps | dhs | w1s | cs | red   (red in a region of its own: nothing
  //              the conv gradient still reads is under it, so no barrier ahead of its stores)
  //   W1 role    head | pt | dht | ared
  static_assert(!SPLIT || (W16 && AUXD), "the roles build on the 16-wave mapping with dps in its own region");
  const int PTB = PP * 32 * HP * 2, DHTB = 2 * HID * HP * 2, DHSB = 2 * CH * HP * 2, DPSB = CH * KD * 4;
  const int o_head = SPLIT ? 0 : XS_BYTES, o_xs = SPLIT ? HEAD_BYTES : 0;
  const int o_dps = SPLIT ? HEAD_BYTES + XS_BYTES : XS_BYTES + (AUXD ? HEAD_BYTES : 0);
  const int o_pt = SPLIT ? HEAD_BYTES : XS_BYTES + RB, o_dht = o_pt + PTB;
  const int o_dhs = SPLIT ? o_dps + DPSB : o_dht + DHTB, o_w1s = o_dhs + DHSB, o_cs = o_w1s + PTB;
  const int o_red = SPLIT ? o_cs + CSB : o_pt, o_ared = SPLIT ? o_dht + DHTB : o_dps;
  float* xs = reinterpret_cast<float*>(smem + o_xs);                       // [CH][XR][28]
  float* dps = reinterpret_cast<float*>(smem + o_dps);                     // [CH][KD] (after the head)
  uint16_t* pt = reinterpret_cast<uint16_t*>(smem + o_pt);                 // [PP*32][HP]
  uint16_t* dht = reinterpret_cast<uint16_t*>(smem + o_dht);               // [2][HID][HP] dh^T hi, lo
  uint16_t* dhs = reinterpret_cast<uint16_t*>(smem + o_dhs);               // [2][CH][HP]  dh hi, lo
  uint16_t* w1s = reinterpret_cast<uint16_t*>(smem + o_w1s);               // [PP*32][HP]
  uint8_t* cs = reinterpret_cast<uint8_t*>(smem + o_cs);                   // [CH][KC] argmax codes (CGP: entries)
  float* red = reinterpret_cast<float*>(smem + o_red);  // [16][320] reduction scratch, after the MFMAs
  // head scratch (aliases dps unless AUXD: used before the dP MFMA of each chunk)
  float* hs = reinterpret_cast<float*>(smem + o_head);  // [CH][HPITCH] h = relu(dense-1)
  float* spl = hs + CH * HPITCH;   // [716] b1[64] W2[64][10] b2[10]
  float* zs = spl + 716;           // [CH][ZP] logits, then dz
  float* rl = zs + CH * ZP;        // [CH] per-row loss
  float* rc = rl + CH;             // [CH] per-row correct
  float* db1p = rc + CH;           // [16][64] db1 partials
  int* ylds = reinterpret_cast<int*>(db1p + 16 * HID);  // [CH] label of the row, -1 if invalid
  const int r0 = 2 * (p0 / PO);
  const int nrows = 2 * ((p1 - 1) / PO) + 4 - r0;
  const int wave = tid >> 6, lane = tid & 63;
  const int ko = 8 * (lane >> 4), lr16 = lane & 15;

  // ---- this block's aux elements ----
  // (auxm, from the host: chunk_aux | log2(threads per element) << 16 -- the divisions
  // that derive them from the grid cost ~40 VALU of the prologue on the device)
  const int chunk_aux = auxm & 0xffff, ltpe = auxm >> 16, tpe = 1 << ltpe;
  const int ae_local = tid >> ltpe, aq = tid & (tpe - 1);
  const int ae = s * chunk_aux + ae_local;
  const bool aux_on = rw1 && ae_local < chunk_aux && ae < NAUX2;
  const int aec = min(ae, NAUX2 - 1);
  float arsum = 0.f;

  // ---- prologue: first the loads whose addresses do not depend on the ctrl block (the
  // previous metric, b1/W2/b2, the bf16 W1 slice, chunk 0's pooled tile and argmax codes),
  // kept ahead of the ctrl load by a scheduling barrier (as in fwd) ----
  // previous step's reduced metric (sharded: fwd folds it from the small messages)
  const float ag_old = sh || !rw1 ? 0.f : Gr[OFF_LOSS + max(0, min(aec - NSMALL, 2))];
  // small parameters (b1/W2/b2, updated by fwd): 2 per thread, re-staged every chunk
  // (16 waves: one per thread, threads past the 714 load nothing)
  float spv0 = 0.f, spv1 = 0.f;
  if (!W16 || tid < NSMALL) spv0 = P[OFF_B1 + tid];
  if (!W16 && tid + 512 < NSMALL) spv1 = P[OFF_B1 + tid + 512];
  // hacc row (tid >> 3), columns 8 (tid & 7) .. + 8; 16 waves: row (tid >> 4), columns
  // 4 (tid & 15) .. + 4 in hq0 / hq1
  constexpr int HQS = W16 ? 4 : 3, HQN = W16 ? 2 : 4;  // log2(threads per row), 16-byte units per thread
  uint4 hq0, hq1, hq2, hq3;
  // known parity (single chunk): the head's first operand -- this step's dense-1 sums --
  // right behind b1 / W2 / b2, before the ctrl block
  const bool hq_early = ONE && phint >= 0;
  auto load_hq = [&](int chunk, int p) __attribute__((always_inline)) {
    const int r = tid >> HQS, q = tid & ((1 << HQS) - 1);
    const int row = min(chunk * CH + r, B - 1);
    const uint4* hp = reinterpret_cast<const uint4*>(hacc + (unsigned)((p * B + row) * HACC_PITCH + q * 2 * HQN));
    hq0 = hp[0];
    hq1 = hp[1];
    if (HQN > 2) {
      hq2 = hp[2];
      hq3 = hp[3];
    } else {
      hq2 = hq3 = make_uint4(0u, 0u, 0u, 0u);
    }
  };
  if (hq_early) load_hq(0, phint);
  const int n8 = K * HID / 8;
  uint4 wv0, wv1;
  // (only in-range units are loaded: clamped duplicates cost load bandwidth -- at PP = 2 the
  // whole second unit is out of range)
  // (conditional loads, not selects between pointers: see fwd's bq)
  // W1 slice units wt and wt + WS: all threads, or (16 waves) waves 12-15 with two each
  constexpr int WS = W16 ? 256 : 512;
  const int wt = W16 ? tid - 768 : tid;  // (< 0: no W1 units)
  wv0 = wv1 = make_uint4(0u, 0u, 0u, 0u);
  // (the bf16 copy has one buffer per step parity: dP reads the live one, the eager update
  // writes the other.  Known parity: the host passed them as w1bf / w1bf_out; else they are
  // buffers 0 / 1 and the load waits for the ctrl block's parity.  W1 role: no bf16 slice)
  auto load_wv = [&](const uint16_t* src) __attribute__((always_inline)) {
    if (!rconv) return;
    if (wt >= 0 && wt < n8) wv0 = reinterpret_cast<const uint4*>(src + p0 * 32 * HID)[wt];
    if ((!SPEC || WS < PP * 32 * HID / 8) && wt >= 0 && wt + WS < n8)
      wv1 = reinterpret_cast<const uint4*>(src + p0 * 32 * HID)[wt + WS];
  };
  if (phint >= 0) load_wv(w1bf);
  // the body -- pooled tile, argmax codes, input rows, read only by the MFMAs and the conv
  // gradient -- is staged by NB threads with two slots each: all 512 when chunked; in the
  // single-chunk step only waves 4-7 (slots bt and bt + 256), which have no logits to
  // compute and store it while waves 0-3 run the logits / softmax (staged by waves 0-3 too,
  // it sat on the head's critical path).  16 waves: the pooled tile and the input rows on
  // waves 4-11, one slot per thread (NB = 512); the argmax codes on waves 12-15 (slot ct)
  constexpr int NB = W16 ? 512 : ONE ? 256 : 512;
  const int bt = ONE ? tid - 256 : tid;  // (< 0: no body slots)
  const bool bw = !ONE || (bt >= 0 && bt < NB);
  const int ct = W16 ? tid - 768 : bt;   // code slot
  // (a role per block: the pooled tile is the W1 role's, the codes and the input rows the conv role's)
  const bool bwp = bw && rw1, bwx = bw && rconv;
  const bool cw = (W16 ? ct >= 0 : bw) && rconv;
  XStage<U8> xst, xst1;      // input rows: slot bt, and (single chunk, 8 waves) bt + 256
  uint4 pv0, pv1, pv2, pv3;  // pooled tile units bt + j NB (K * 8 <= 1024 units)
  uint4 cv, cv1;             // argmax codes, units ct (+ NB), zeroed at the LDS store unless cok
  bool cok = false, cok1 = false;
  int ylab = 0;
  bool yval = false;
  const int BP = (B + CH - 1) / CH * CH;
  const int kc = K / 16;  // = 2 np, np in 1..MAXPP
  // (constant configuration) pooled-tile slots a body thread needs, 16-byte code units per image
  constexpr int NPV = SPEC ? (C::PP * 32 * 8 + NB - 1) / NB : 4, KCM = SPEC ? 2 * C::PP : 1;
  // i / kc for i < 512 without a division sequence: (i / 2) / np, np = 3 by a multiply
  auto div_kc = [&](int i) __attribute__((always_inline)) {
    return np == 3 ? (int)(((unsigned)(i >> 1) * 21846u) >> 16) : (i >> 1) >> (np >> 1);
  };
  static_assert(MAXPP == 4, "div_kc covers np = 1..4");
  // (32-bit element offsets: the pooled tile is FEAT x BP bf16, far below 2^31; only
  // in-range units load -- conditional loads, not pointer selects, see fwd's bq)
  auto load_pv = [&](uint4& v, int i, int chunk) __attribute__((always_inline)) {
    v = make_uint4(0u, 0u, 0u, 0u);
    if (i < K * 8) v = *reinterpret_cast<const uint4*>(pooled + (__umul24(p0 * NF + (i >> 3), BP) + chunk * CH + (i & 7) * 8));
  };
  // (constant configuration: unit i = image i / KCM, 16 codes q = i % KCM; units past the
  // short last slice are not loaded and staged as zeros)
  auto load_cv = [&](uint4& v, bool& ok, int i, int chunk) __attribute__((always_inline)) {
    if constexpr (SPEC) {
      const int bb = i / KCM, q = i - bb * KCM;
      ok = i < CH * KCM && q < kc;
      v = make_uint4(0u, 0u, 0u, 0u);
      if (ok) v = *reinterpret_cast<const uint4*>(code + (__umul24(bb, FEAT) + p0 * NF + q * 16));
      return;
    }
    const int bb = div_kc(i), q = i - bb * kc, lb = chunk * CH + bb;
    ok = i < CH * kc && lb < B;
    v = make_uint4(0u, 0u, 0u, 0u);
    if (i < CH * kc) v = *reinterpret_cast<const uint4*>(code + (__umul24(min(lb, B - 1), FEAT) + p0 * NF + q * 16));
  };
  auto load_indep = [&](int chunk) __attribute__((always_inline)) {
    if (bwp) {
      load_pv(pv0, bt, chunk);
      if (NPV > 1) load_pv(pv1, bt + NB, chunk);
      if (ONE && NPV > 2) {
        load_pv(pv2, bt + 2 * NB, chunk);
        load_pv(pv3, bt + 3 * NB, chunk);
      }
    }
    if (cw) {
      load_cv(cv, cok, ct, chunk);
      if (ONE && !W16 && (!SPEC || NB < CH * KCM)) load_cv(cv1, cok1, ct + NB, chunk);
    }
    if (ycur != nullptr) {  // labels and rows as this step's fwd read them: no cursor needed
      const int b = chunk * CH + min(tid, CH - 1);
      ylab = ycur[min(b, B - 1)];
      yval = tid < CH && b < B && ylab >= 0;
      if (bwx) {
        x_load<U8>(xst, xcur, chunk * CH, B, B - chunk * CH, LG_CH, r0, nrows, bt);
        if (ONE && !W16) x_load<U8>(xst1, xcur, chunk * CH, B, B - chunk * CH, LG_CH, r0, nrows, bt + NB);
      }
    }
  };
  load_indep(0);
  __builtin_amdgcn_sched_barrier(0);

  const Ctrl c = *ctrl;
  const int cur = c.cur2, par = phint >= 0 ? phint : c.par2;
  if (phint >= 0 && phint != c.par2 && blk0 && tid == 0)
    __hip_atomic_fetch_or(&ctrl->bad, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // parity unknown to the host: w1bf / w1bf_out are buffers 0 / 1, the live one is `par`
  if (phint < 0 && par) {
    const uint16_t* live = w1bf_out;
    w1bf_out = const_cast<uint16_t*>(w1bf);
    w1bf = live;
  }
  if (phint < 0) load_wv(w1bf);
  const unsigned xe = (unsigned)c.xcnt2 + 1u;  // sharded: this step's exchange epoch
  if (blk0 && tid == 0) {
    ctrl->cursor = next_cursor(c, cur);
    ctrl->iterations = c.iterations + 1;
    ctrl->wpar = c.wpar ^ 1;  // fwd of this step wrote the next W1 buffer
    ctrl->pending = 1;
    if (sh) ctrl->xcnt = (int)xe;
  }
  const long gstart = (long)cur * c.global_batch;
  const long row_base = gstart + c.row0;
  const int gcount = (int)min((long)c.global_batch, (long)c.nsamples - gstart);
  const float inv = gcount > 0 ? 1.f / (float)gcount : 0.f;
  // next-batch prefetch for the next fwd: this block's share of the next step's rows as
  // 16-byte units (stored at the end; the loads travel meanwhile)
  const int ncur = next_cursor(c, cur);
  constexpr int UPI = U8 ? NPIX / 16 : NPIX / 4;  // 16-byte units per image
  // (a block's 512 units sit on threads 0-511, as does its share of the dead hacc parity)
  const int xpu = s * 512 + tid;
  const bool xpf = ONE && rw1 && xnext != nullptr && (!W16 || tid < 512) && xpu < B * UPI;
  uint4 xnv = make_uint4(0u, 0u, 0u, 0u);

  // then the ctrl-dependent ones: the dense-1 sums by parity (unless known), the labels and
  // the batch rows (unless the fwd staged them in ycur / xcur)
  auto load_dep = [&](int chunk) __attribute__((always_inline)) {
    if (!hq_early || chunk > 0) load_hq(chunk, par);
    if (ycur == nullptr) {
      {
        const int b = chunk * CH + min(tid, CH - 1);
        const long g = row_base + b;
        yval = tid < CH && b < B && g < c.nsamples;
        ylab = labels[max(0L, min(g, (long)c.nsamples - 1))];
      }
      if (bwx) {
        x_load<U8>(xst, X, row_base + chunk * CH, c.nsamples, B - chunk * CH, LG_CH, r0, nrows, bt);
        if (ONE && !W16) x_load<U8>(xst1, X, row_base + chunk * CH, c.nsamples, B - chunk * CH, LG_CH, r0, nrows, bt + NB);
      }
    }
  };
  auto load_chunk = [&](int chunk) __attribute__((always_inline)) {
    load_indep(chunk);
    load_dep(chunk);
  };
  // what the head needs (b1 / W2 / b2, labels) and what only the MFMAs / conv gradient
  // need (pooled tile, argmax codes, input rows): the single-chunk backward stores the
  // latter while waves 0-3 run the logits / softmax, so the head does not wait for the
  // input rows (the largest, last-issued loads)
  auto store_head = [&]() __attribute__((always_inline)) {
    if (!W16 || tid < NSMALL) spl[tid] = spv0;
    if (!W16 && tid + 512 < NSMALL) spl[tid + 512] = spv1;
    if (tid < CH) ylds[tid] = yval ? ylab : -1;
  };
  auto store_pv = [&](const uint4& v, int i) __attribute__((always_inline)) {
    // (constant configuration: every row of the tile, rows past K as the zeros loaded)
    if (i < (SPEC ? PP * 32 * 8 : K * 8)) *reinterpret_cast<uint4*>(pt + (i >> 3) * HP + (i & 7) * 8) = v;
  };
  auto store_cv = [&](const uint4& v, bool ok, int i) __attribute__((always_inline)) {
    if constexpr (CGP) {
      // 16 codes -> 16 entries (code_entries); a unit that was not loaded -- the short last
      // slice's positions >= NPOS -- as code 0: off, offset 0
      const int bb = i / KCM, q = i - bb * KCM;
      const uint32_t w[4] = {ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u};
      uint32_t e[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) code_entries(w[k], e[2 * k], e[2 * k + 1]);
      if (i < CH * KCM) {
        uint4* dst = reinterpret_cast<uint4*>(cs + (bb * KC + q * 16) * CGE_BYTES);
        dst[0] = make_uint4(e[0], e[1], e[2], e[3]);
        dst[1] = make_uint4(e[4], e[5], e[6], e[7]);
      }
      return;
    }
    if constexpr (SPEC) {
      const int bb = i / KCM, q = i - bb * KCM;
      if (i < CH * KCM) *reinterpret_cast<uint4*>(cs + bb * KC + q * 16) = ok ? v : make_uint4(0u, 0u, 0u, 0u);
      return;
    }
    if (i < CH * kc) {
      const int bb = div_kc(i), q = i - bb * kc;
      *reinterpret_cast<uint4*>(cs + bb * KC + q * 16) = ok ? v : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto store_body = [&]() __attribute__((always_inline)) {
    if (cw) {
      store_cv(cv, cok, ct);
      if (ONE && !W16 && (!SPEC || NB < CH * KCM)) store_cv(cv1, cok1, ct + NB);
    }
    if (bwp) {
      store_pv(pv0, bt);
      if (NPV > 1) store_pv(pv1, bt + NB);
      if (ONE && NPV > 2) {
        store_pv(pv2, bt + 2 * NB);
        store_pv(pv3, bt + 3 * NB);
      }
    }
    if (bwx) {
      x_store<U8>(xst, xs, LG_CH, nrows);
      if (ONE && !W16) x_store<U8>(xst1, xs, LG_CH, nrows);
    }
  };
  auto store_chunk = [&](int chunk) __attribute__((always_inline)) {
    store_body();
    store_head();
  };
  load_dep(0);
  // the next step's rows for its fwd (issued after this step's own loads: in-order vmcnt)
  if (xpf) {
    const int b = xpu / UPI, q = xpu - b * UPI;
    const int g = (int)((long)ncur * c.global_batch + c.row0) + b;  // (dataset < 2^31 bytes: 32-bit)
    if (g < c.nsamples)
      xnv = reinterpret_cast<const uint4*>(static_cast<const char*>(X) + __umul24((unsigned)g, U8 ? NPIX : 4 * NPIX))[q];
  }
  // (w1s is read only by the dP MFMAs, several barriers later)
  // (constant configuration: every row of the tile is written, rows past K as the zeros held)
  const int n8s = SPEC ? PP * 32 * HID / 8 : n8;
  if (rconv && wt >= 0 && wt < n8s) *reinterpret_cast<uint4*>(w1s + (wt >> 3) * HP + (wt & 7) * 8) = wv0;
  if (rconv && wt >= 0 && wt + WS < n8s) *reinterpret_cast<uint4*>(w1s + ((wt + WS) >> 3) * HP + (wt & 7) * 8) = wv1;

  // dW1 / dP tiles of the wave: 8 waves, tile rows dm0 + 2 i (one per position i); 16 waves,
  // the one tile row dm0 = wave >> 2 (position dm0 >> 1)
  constexpr int TPW = W16 ? 1 : MAXPP;
  const int dn = wave & 3, dm0 = wave >> 2;
  const bool mom = c.momentum != 0.f;
  float ew[ONE ? MAXPP : 1][4], ev[ONE ? MAXPP : 1][4];  // eager (single chunk only)
  f32x4 accw[MAXPP];
#pragma unroll
  for (int i = 0; i < MAXPP; ++i) accw[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // ---- sharded exchange: this wave's dW1 tiles form half of unit u = 4 s + dn (rows of
  // tiles dm0 + 2 i, 16 columns), owned by rank u % world ----
  const int NU = 4 * NS, xu = 4 * s + dn;
  const int xo = !sh ? 0 : (xa.world & (xa.world - 1)) == 0 ? xu & (xa.world - 1) : xu % xa.world;
  const bool xown = sh && xo == xa.rank;
  auto push_partials = [&]() __attribute__((always_inline)) {
    if (!sh || xown) return;
    float* slot = xa.in[xo] + ((long)xa.rank * NU + xu) * kXPSlot;
    if (xa.gbf16) {  // bf16 partials: half the bytes (the owner accumulates in fp32)
      uint2* dst = reinterpret_cast<uint2*>(slot) + dm0 * MAXPP * 64 + lane;
#pragma unroll
      for (int i = 0; i < MAXPP; ++i)
        if (i < np) dst[i * 64] = pack_bf16x4(accw[i]);
    } else {
      float4* dst = reinterpret_cast<float4*>(slot) + dm0 * MAXPP * 64 + lane;
#pragma unroll
      for (int i = 0; i < MAXPP; ++i)
        if (i < np) dst[i * 64] = make_float4(accw[i][0], accw[i][1], accw[i][2], accw[i][3]);
    }
  };
  // conv gradient: channel ch, image group grp (4 images); 16 waves: threads 0-511 accumulate
  // taps 0-4, threads 512-1023 taps 5-8 and the bias sum (T0 .. T1 of this thread)
  const int ch = tid & 31, grp = (tid >> 5) & 15, half = tid >> 9;
  float gw[9], gb = 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) gw[t] = 0.f;
  // this block's aux elements over the chunk's rows (fixed order: deterministic); they read
  // the head scratch only (hs, zs, rl, rc, db1p)
  auto aux_sums = [&]() __attribute__((always_inline)) {
    if (!aux_on) return;
    // element order = parameter order of b1[64], W2[64][10], b2[10] (G + OFF_B1)
    float a = 0.f;
    if (aec < HID) {
      if (aq == 0)
#pragma unroll
        for (int q = 0; q < 16; ++q) a += db1p[q * HID + aec];
    } else if (aec < HID + HID * NCLS) {
      const int kk = (aec - HID) / NCLS, cc = aec - HID - kk * NCLS;
      for (int r = aq; r < CH; r += tpe) a = fmaf(hs[r * HPITCH + kk], zs[r * ZP + cc], a);
    } else if (aec < NSMALL) {
      const int cc = aec - HID - HID * NCLS;
      for (int r = aq; r < CH; r += tpe) a += zs[r * ZP + cc];
    } else if (aec < NSMALL + 2) {
      const float* src = aec == NSMALL ? rl : rc;
      for (int r = aq; r < CH; r += tpe) a += src[r];
    }
    arsum += a;
  };
  const int nchunks = ONE ? 1 : (B + CH - 1) / CH;

  for (int chunk = 0; chunk < nchunks; ++chunk) {
    if (chunk) {
      lds_barrier();
      load_chunk(chunk);
    }
    if (ONE) store_head();
    else store_chunk(chunk);
    lds_barrier();
    stamp(sts, st, 1);
    // eager: the slice's fp32 masters / velocities for the update right after the dW1
    // MFMAs, issued once the staged operands have landed (in flight through the head)
    if (ONE && eager && rw1) {
#pragma unroll
      for (int i = 0; i < TPW; ++i) {
        const int mt = W16 ? dm0 : dm0 + 2 * i, pi = W16 ? dm0 >> 1 : i;  // tile row, its position
        if (pi >= npl) break;
        if (SPEC && pi >= np) continue;  // (short last slice: nothing to update)
        // (one address per tile, the 4 rows at immediate offsets)
        const unsigned e0 = OFF_W1 + (unsigned)((p0 * 32 + 16 * mt + 4 * (lane >> 4)) * HID + 16 * dn + lr16);
        const float* pw = Pw + e0;
        const float* vw = Vw + e0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ew[i][j] = pw[j * HID];
          ev[i][j] = mom ? vw[j * HID] : 0.f;
        }
      }
    }
    // ---- head (every block, redundantly): h = relu(hacc / 2^32 + b1) ----
    {
      const int r = tid >> HQS, q = tid & ((1 << HQS) - 1);
      const bool rv = chunk * CH + r < B;
      const uint4 hq[4] = {hq0, hq1, hq2, hq3};
      long long hq64[2 * HQN];
      float hf[2 * HQN];
#pragma unroll
      for (int u = 0; u < HQN; ++u) {
        hq64[2 * u] = (long long)(((unsigned long long)hq[u].y << 32) | hq[u].x);
        hq64[2 * u + 1] = (long long)(((unsigned long long)hq[u].w << 32) | hq[u].z);
      }
      // (every thread of the block is here: the wave-uniform test sees whole waves)
      if constexpr (C::FIXW) {
        from_fix_wave(hf, hq64, HINV);
      } else {
#pragma unroll
        for (int i = 0; i < 2 * HQN; ++i) hf[i] = from_fix(hq64[i], HINV);
      }
#pragma unroll
      for (int i = 0; i < 2 * HQN; ++i) {
        const int n = q * 2 * HQN + i;
        hs[r * HPITCH + n] = rv ? fmaxf(hf[i] + spl[n], 0.f) : 0.f;
      }
    }
    lds_barrier();
    stamp(sts, st, 6);
    if (ONE && wave >= 4) {  // (the waves without a logits tile stage the whole body: see NB above)
      store_body();
      stamp(sts, st, 12);
    }
    // logits on f32 MFMA (wave mt: rows 16 mt .. 16 mt + 15, 16 columns, 10 used), then
    // softmax-xent / accuracy / dz over each row's 16 lanes (DPP row reductions); the four
    // rows j of a lane are independent chains, interleaved
    if (wave < 4) {
      const int mt = wave, lr = lane & 15, kq = lane >> 4;
      float av[HID / 4], bv[HID / 4];  // all operands first: one LDS wait, then 16 MFMAs
#pragma unroll
      for (int ks = 0; ks < HID / 4; ++ks) {
        const int k = 4 * ks + kq;
        av[ks] = hs[(16 * mt + lr) * HPITCH + k];
        bv[ks] = spl[HID + k * NCLS + min(lr, NCLS - 1)];
      }
      // the labels of this lane's 4 rows, read with the operands (read after the softmax, they
      // were 4 serial LDS round trips on the critical path)
      int yv4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) yv4[j] = ylds[16 * mt + 4 * kq + j];
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      if (ONE) stamp(sts, st, 9);  // (sub-phase stamps, single chunk: wave 0's view)
#pragma unroll
      for (int ks = 0; ks < HID / 4; ++ks) acc = mfma4(av[ks], lr < NCLS ? bv[ks] : 0.f, acc);
      const float b2v = lr < NCLS ? spl[HID + HID * NCLS + lr] : 0.f;
      float v[4], m[4], e[4], lse[4];
      int am[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = lr < NCLS ? acc[j] + b2v : -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) m[j] = row16_max(v[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = lr < NCLS ? __expf(v[j] - m[j]) : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = row16_sum(e[j]);
      if (ONE) stamp(sts, st, 10);
      // log-sum-exp: the sum is in [1, 10], so the hardware log2 (v_log_f32) is accurate here;
      // __logf's denormal-safe expansion was ~15 instructions per row on the critical path
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lse[j] = m[j] + __builtin_amdgcn_logf(e[j]) * 0.693147180559945f;
        am[j] = row16_min(v[j] == m[j] ? lr : 16);
      }
      if (ONE) stamp(sts, st, 11);
      // dz for all 16 lanes of a row (lanes >= NCLS: v = -inf, so 0 -- the padding of the
      // zs row), no per-store exec masks; the label's lane writes the row's loss and hit
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = 16 * mt + 4 * kq + j;
        const int yv = yv4[j];
        const bool valid = yv >= 0;
        const int y = valid ? yv : 0;
        zs[r * ZP + lr] = valid ? (__expf(v[j] - lse[j]) - (lr == y ? 1.f : 0.f)) * inv : 0.f;
        if (lr == y) {
          rl[r] = valid ? (lse[j] - v[j]) : 0.f;
          rc[r] = (valid && am[j] == y) ? 1.f : 0.f;
        }
      }
    }
    if (ONE && wave < 4) stamp(sts, st, 12);
    lds_barrier();
    stamp(sts, st, 7);
    // dh = (dz W2^T) * [h > 0] on f32 MFMA: 16 tiles of 16x16, two per wave, K = 10 (three
    // k-steps of 4, zero-padded); a lane's 4 outputs are 4 consecutive rows of one column,
    // so dh^T is stored 8 bytes at a time.
    // Every LDS operand of both tiles first (dz, W2, the ReLU mask of h): one LDS wait
    // instead of three per tile -- hipcc cannot move reads above the tile's dh stores itself
    constexpr int NDH = 16 / NW;  // (16 waves: tile = wave)
    float za[NDH][3], wb[NDH][3], hm[NDH][4];
#pragma unroll
    for (int ti = 0; ti < NDH; ++ti) {
      const int t = wave + 8 * ti, mt = t >> 2, nt = t & 3, lr = lane & 15, kq = lane >> 4;
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) {
        const int k = 4 * ks + kq;
        za[ti][ks] = k < NCLS ? zs[(16 * mt + lr) * ZP + k] : 0.f;
        wb[ti][ks] = k < NCLS ? spl[HID + (16 * nt + lr) * NCLS + k] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) hm[ti][j] = hs[(16 * mt + 4 * kq + j) * HPITCH + 16 * nt + lr];
    }
#pragma unroll
    for (int ti = 0; ti < NDH; ++ti) {
      const int t = wave + 8 * ti, mt = t >> 2, nt = t & 3, lr = lane & 15, kq = lane >> 4;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 3; ++ks) acc = mfma4(za[ti][ks], wb[ti][ks], acc);
      const int n = 16 * nt + lr, rb = 16 * mt + 4 * kq;
      uint16_t hi[4], lo[4];
      float dsum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = hm[ti][j] > 0.f ? acc[j] : 0.f;
        dsum += d;
        hi[j] = f2bf(d);
        lo[j] = bf16_lo(d, hi[j]);
        if (rconv) {  // (a role per block: only the layout the role's MFMAs read)
          dhs[(rb + j) * HP + n] = hi[j];
          dhs[CH * HP + (rb + j) * HP + n] = lo[j];
        }
      }
      if (rw1) {
        *reinterpret_cast<uint2*>(dht + n * HP + rb) =
            make_uint2((uint32_t)hi[0] | ((uint32_t)hi[1] << 16), (uint32_t)hi[2] | ((uint32_t)hi[3] << 16));
        *reinterpret_cast<uint2*>(dht + HID * HP + n * HP + rb) =
            make_uint2((uint32_t)lo[0] | ((uint32_t)lo[1] << 16), (uint32_t)lo[2] | ((uint32_t)lo[3] << 16));
        db1p[(4 * mt + kq) * HID + n] = dsum;  // [16][64]: partial over rows rb .. rb + 3
      }
    }
    if (st != nullptr) wst_dh = __builtin_amdgcn_s_memrealtime();  // (this wave's arrival at the dh barrier)
    lds_barrier();
    stamp(sts, st, 8);
    if (!AUXD) {
      aux_sums();
      lds_barrier();  // the head scratch (dps) is overwritten by dP below
    }
    stamp(sts, st, 2);
    // dW1[k][n] += sum_b P[b][k] (dh_hi + dh_lo)[b][n]
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      if (!rw1) break;
      const int mt = W16 ? dm0 : dm0 + 2 * i;
      if ((W16 ? dm0 >> 1 : i) >= npl) break;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const bf16x8 a = ld_frag(pt + (16 * mt + lr16) * HP + kk * 32 + ko);
        const bf16x8 bh = ld_frag(dht + (16 * dn + lr16) * HP + kk * 32 + ko);
        const bf16x8 bl = ld_frag(dht + HID * HP + (16 * dn + lr16) * HP + kk * 32 + ko);
        accw[i] = mfma16(a, bh, accw[i]);
        accw[i] = mfma16(a, bl, accw[i]);
      }
    }
    // sharded: a unit owned by another rank leaves now (data only; its flag is raised once
    // the stores have drained, after the conv gradient) and travels during dP / conv grad
    if (ONE && sh) push_partials();
    // eager: the slice's SGD update now, its stores overlapping dP and the conv gradient
    // (fp32 master and velocity in place: only this block touches the slice's masters in this
    // launch; the bf16 copy for the next fwd goes to the buffer of the other parity, which no
    // block of this launch reads -- the slice's conv-role block reads the live one)
    if (ONE && eager && rw1) {
#pragma unroll
      for (int i = 0; i < TPW; ++i) {
        const int mt = W16 ? dm0 : dm0 + 2 * i, pi = W16 ? dm0 >> 1 : i;
        if (pi >= npl) break;
        if (SPEC && pi >= np) continue;
        const unsigned e0 = OFF_W1 + (unsigned)((p0 * 32 + 16 * mt + 4 * (lane >> 4)) * HID + 16 * dn + lr16);
        float* pw = Pw + e0;
        float* vw = Vw + e0;
        uint16_t* bw = w1bf_out + (e0 - OFF_W1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float wn, vn;
          sgd_update(ew[i][j], accw[i][j], ev[i][j], c.lr, c.momentum, c.nesterov, wn, vn);
          pw[j * HID] = wn;
          if (mom) vw[j * HID] = vn;
          bw[j * HID] = f2bf(wn);
        }
      }
    }
    if (SPLIT && !rconv) stamp(sts, st, 3);  // (W1 role: update stored -- its stores issued)
    // dP[b][k] = sum_n (dh_hi + dh_lo)[b][n] W1[k][n]
    if (rconv) {
      const int pm = wave & 3;
#pragma unroll
      for (int i = 0; i < TPW; ++i) {
        if (!W16 && i >= npl) break;
        const int nt = W16 ? wave >> 2 : (wave >> 2) + 2 * i;
        f32x4 a4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const bf16x8 ah = ld_frag(dhs + (16 * pm + lr16) * HP + kk * 32 + ko);
          const bf16x8 al = ld_frag(dhs + CH * HP + (16 * pm + lr16) * HP + kk * 32 + ko);
          const bf16x8 bb = ld_frag(w1s + (16 * nt + lr16) * HP + kk * 32 + ko);
          a4 = mfma16(ah, bb, a4);
          a4 = mfma16(al, bb, a4);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) dps[(16 * pm + 4 * (lane >> 4) + j) * KD + 16 * nt + lr16] = a4[j];
      }
    }
    if (C::AUX == 1) aux_sums();  // (behind the MFMAs and the dP stores, nothing waits for it)
    if (st != nullptr) wst_cg = __builtin_amdgcn_s_memrealtime();  // (arrival at the pre-conv-gradient barrier)
    if (SPLIT && !rconv) break;  // (W1 role: no dps, no conv gradient; single chunk)
    lds_barrier();
    stamp(sts, st, 3);
    // MaxPool + ReLU backward fused into the conv weight-gradient accumulation: taps T0 .. T1 - 1
    // of this thread (all nine, or the half's), the bias sum with the last tap
    auto conv_grad = [&](auto t0c, auto t1c) __attribute__((always_inline)) {
      constexpr int T0 = decltype(t0c)::value, T1 = decltype(t1c)::value;
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int bb = grp * 4 + ii;
        for (int pl = 0; pl < npl; ++pl) {
          // (short last slice: the rows of a position >= NPOS were never staged -- no 0 x garbage)
          if (SPEC && pl >= np) continue;
          const int cd = cs[bb * KC + pl * 32 + ch];
          const int pos = p0 + pl, py = pos / PO, px = pos - py * PO;
          const float dv0 = dps[bb * KD + pl * 32 + ch];
          const float d = (cd & 4) ? dv0 : 0.f;
          const int y0 = 2 * py + ((cd >> 1) & 1) - r0, x0 = 2 * px + (cd & 1);
          const float* xp = xs + (bb * XR + y0) * IMG + x0;
          float xv[9];
#pragma unroll
          for (int t = T0; t < T1; ++t) xv[t] = xp[(t / 3) * IMG + (t % 3)];
#pragma unroll
          for (int t = T0; t < T1; ++t) gw[t] = fmaf(d, xv[t], gw[t]);
          if (T1 == 9) gb += d;
        }
      }
    };
    // The same sums from the pre-decoded entries (CGP, see code_entries): conv_grad spends most
    // of its VALU stream on decoding and address arithmetic, per pair and behind a full LDS wait
    // each, and the phase is VALU-issue bound.  Here a pair costs an address add and the mask
    // `and`: the entry's offset byte is added to a per-thread base (image group and position
    // folded in, the position's (py, px) part scalar), image and tap steps are immediate
    // offsets; the loads come in two batches -- every entry and dP value, then every x tap --
    // and the fmaf chains run in conv_grad's order (image outer, position inner, taps ascending).
    // Positions >= NPOS of the short last slice are not skipped: their entries are `off` (d = +0,
    // as for any unit that was off), their base is the slice's last real position, so every x read
    // is of staged, finite rows and fmaf(+0, x, g) leaves g (never -0) as it is.
    auto conv_grad_pre = [&](auto t0c, auto t1c) __attribute__((always_inline)) {
      constexpr int T0 = decltype(t0c)::value, T1 = decltype(t1c)::value, NPL = SPEC ? C::PP : 1;
      const uint8_t* ce = cs + (grp * 4 * KC + ch) * CGE_BYTES;
      const float* dp = dps + grp * 4 * KD + ch;
      uint32_t eo[4][NPL];
      int em[4][NPL];
      float dv[4][NPL];
#pragma unroll
      for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
          eo[ii][pl] = ce[(ii * KC + pl * 32) * CGE_BYTES];
          em[ii][pl] = reinterpret_cast<const int8_t*>(ce)[(ii * KC + pl * 32) * CGE_BYTES + 1];
          dv[ii][pl] = dp[ii * KD + pl * 32];
        }
      const char* xg = reinterpret_cast<const char*>(xs) + grp * (4 * XR * IMG * 4);
      float xv[4][NPL][T1 - T0];
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) {
        const int pos = min(p0 + pl, NPOS - 1), py = pos / PO, px = pos - py * PO;
        const char* xb = xg + ((2 * py - r0) * IMG + 2 * px) * 4;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
          const float* xp = reinterpret_cast<const float*>(xb + eo[ii][pl]);
#pragma unroll
          for (int t = T0; t < T1; ++t) xv[ii][pl][t - T0] = xp[ii * XR * IMG + (t / 3) * IMG + (t % 3)];
        }
      }
#pragma unroll
      for (int ii = 0; ii < 4; ++ii)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
          const float d = __int_as_float(__float_as_int(dv[ii][pl]) & em[ii][pl]);
#pragma unroll
          for (int t = T0; t < T1; ++t) gw[t] = fmaf(d, xv[ii][pl][t - T0], gw[t]);
          if (T1 == 9) gb += d;
        }
    };
    using std::integral_constant;
    if constexpr (CGP) {
      if (half == 0) conv_grad_pre(integral_constant<int, 0>{}, integral_constant<int, 5>{});
      else conv_grad_pre(integral_constant<int, 5>{}, integral_constant<int, 9>{});
    } else if (!W16) conv_grad(integral_constant<int, 0>{}, integral_constant<int, 9>{});
    else if (half == 0) conv_grad(integral_constant<int, 0>{}, integral_constant<int, 5>{});
    else conv_grad(integral_constant<int, 5>{}, integral_constant<int, 9>{});
  }
  stamp(sts, st, 4);
  if (!ONE && sh) push_partials();
  // ---- dW1 straight into the flat gradient buffer (this block owns these rows), unless
  // the update was applied eagerly above or the exchange carries it ----
#pragma unroll
  for (int i = 0; i < MAXPP; ++i) {
    if (i >= np || (ONE && eager) || sh) break;
    const int mt = dm0 + 2 * i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 16 * mt + 4 * (lane >> 4) + j;
      G[OFF_W1 + (unsigned)((p0 * 32 + k) * HID + 16 * dn + lr16)] = accw[i][j];
    }
  }
  // pt/dht region becomes `red`, dps becomes `ared` (a role per block: both have regions of
  // their own, which nothing read since the last barrier lies under)
  if (!SPLIT) lds_barrier();
  // (16 waves: each half writes the taps it accumulated; red holds the same values either way)
  if (rconv) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
      if (!W16 || half == (t >= 5 ? 1 : 0)) red[grp * NCONV + t * NF + ch] = gw[t];
    if (!W16 || half == 1) red[grp * NCONV + OFF_BC + ch] = gb;
  }
  float* ared = reinterpret_cast<float*>(smem + o_ared);
  if (rw1 && (!W16 || tid < 512)) ared[tid] = arsum;  // (aux_split maps 512 threads)
  if (st != nullptr) wst_red = __builtin_amdgcn_s_memrealtime();  // (conv gradient done, its sums stored)
  lds_barrier();
  // this slice's conv-gradient partial, fixed order over the 16 thread groups, then a
  // 64-bit fixed-point atomic add (order-independent sum over the slices)
  for (int i = tid; i < (cprobe || !rconv ? 0 : NCONV); i += NT) {
    float a = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) a += red[r * NCONV + i];
    atomic_add_i64(hconv + par * NCONV + i, to_fix(a, CSCALE, &ctrl->bad));
  }
  // ---- aux: new b1/W2/b2 gradient, metric tail ----
  if (aux_on && aq == 0) {
    float tot = 0.f;
    for (int q = 0; q < tpe; ++q) tot += ared[ae_local * tpe + q];
    if (ae < NSMALL) {
      G[OFF_B1 + ae] = tot;
    } else {
      const int m = ae - NSMALL;  // 0 loss, 1 correct, 2 count
      float* accp = m == 0 ? &ctrl->acc_loss : (m == 1 ? &ctrl->acc_correct : &ctrl->acc_count);
      const float old = m == 0 ? c.acc_loss : (m == 1 ? c.acc_correct : c.acc_count);
      // fold the previous step's all-reduced metric into the epoch total -- if there is one
      // not yet folded: none before the first step, none right after a flush (which folded
      // it), and the staging may hold anything then (the peer self-test's values)
      if (!sh) *accp = c.pend2 ? old + ag_old : old;
      // (a non-finite / out-of-range fixed-point input so far: the loss is NaN from now on)
      G[OFF_LOSS + m] = m == 0 && c.bad ? __builtin_nanf("") : m < 2 ? tot : (float)max(0, min(B, gcount - c.row0));
    }
  }
  // zero the dead hacc parity (read by the previous step's bwd) for the next fwd,
  // spread over the blocks
  {
    long long* hz = hacc + (long)(par ^ 1) * B * HACC_PITCH;
    if (rw1 && (!W16 || tid < 512))
      for (int i = s * 512 + tid; i < B * HID / 2; i += NS * 512)  // (32 16-B units per row)
        *reinterpret_cast<uint4*>(hz + (i >> 5) * HACC_PITCH + (i & 31) * 2) = make_uint4(0u, 0u, 0u, 0u);
  }
  if (xpf) reinterpret_cast<uint4*>(xnext)[xpu] = xnv;
  if (ONE && rw1 && xnext != nullptr && s == 0 && tid == 0) *xtag = ((long long)c.xgen << 32) | (long long)(unsigned)(ncur + 1);
  if (C::SH && sh) exchange_tail(xa, ctrl, G, hconv + par * NCONV, accw, xe, s, NS, np, p0, dn, dm0, lane, tid, xown, xo, xu);
  stamp(sts, st, 5);
  stamp_flush(sts, st, 13);
  if (st != nullptr && tid == 256) st[blockIdx.x * 16 + 13] = sts.t[12];  // wave 4's view
  // the stamps above are wave 0's (slot 13: wave 4's).  Slots 14 / 15: the view of one wave
  // per block (block s: wave s mod NW, so the grid covers every wave ~NS / NW times) of its
  // arrival at the dh barrier and at the pre-conv-gradient barrier; the top byte of slot 14
  // holds that wave, the top byte of slot 15 the waves per block
  if (st != nullptr && tid == 64 * (s % NW)) {
    st[blockIdx.x * 16 + 14] = (wst_dh & 0x00ffffffffffffffull) | ((unsigned long long)(s % NW) << 56);
    st[blockIdx.x * 16 + 15] = (wst_cg & 0x00ffffffffffffffull) | ((unsigned long long)NW << 56);
    // the same wave's arrival at the barrier ahead of the `red` reduction -- the end of its conv
    // gradient (wave 0's slot 4 is stamped when wave 0 gets there, and what it then waits for is
    // the slowest wave).  The 16 slots of a block's row are taken: block b's value goes to slot
    // b & 15 of row nblk + (b >> 4), behind the nblk rows of the grid (<= 170 blocks of 256 rows;
    // nblk a constant in the flagship kernel: gridDim would pull in the hidden kernel arguments)
    const int nblk = SPEC ? (SPLIT ? 2 * NSC : NSC) : (int)gridDim.x;
    st[(nblk + ((int)blockIdx.x >> 4)) * 16 + ((int)blockIdx.x & 15)] =
        (wst_red & 0x00ffffffffffffffull) | ((unsigned long long)(s % NW) << 56);
  }
}

template <bool U8, bool ONE>
// (the first 16 argument dwords arrive preloaded in SGPRs: they are what the prologue's first
// loads address -- the dense-1 sums by the known parity, this step's staged labels / rows, b1 /
// W2 / b2, the bf16 W1 slice, the pooled tile and codes; later arguments come from the
// kernarg segment, a scalar load's latency behind)
__global__ __launch_bounds__(512) void bwd(long long* __restrict__ hacc, const int* __restrict__ ycur,
                                           const void* __restrict__ xcur, int phint, int bpp, const float* P,
                                           const uint16_t* w1bf, const uint16_t* __restrict__ pooled,
                                           const uint8_t* __restrict__ code, Ctrl* __restrict__ ctrl,
                                           const void* __restrict__ X, const int* __restrict__ labels,
                                           float* __restrict__ G, long long* __restrict__ hconv,
                                           int eager, float* Pw, float* Vw, uint16_t* w1bf_out,
                                           unsigned long long* st, const float* __restrict__ Gr, const XArgs xa,
                                           void* __restrict__ xnext, long long* __restrict__ xtag, int auxm) {
  bwd_body<U8, ONE, CfgGeneric>(hacc, ycur, xcur, phint, bpp, P, w1bf, pooled, code, ctrl, X, labels, G, hconv, eager,
                                Pw, Vw, w1bf_out, st, Gr, xa, xnext, xtag, auxm);
}

// The flagship configuration (CfgFlagBwd, single chunk): no packed sizes, no exchange
// arguments; the aux split follows from the constant slicing.  The preloaded dwords are the
// same pointers as above and the parity hint.  Grid CfgFlagBwd::GRID: one block per slice, or
// (SPLIT) two, a role each.  w1bf / w1bf_out: the bf16 W1 pair (see CfgFlagBwd).
template <bool U8>
__global__ __launch_bounds__(CfgFlagBwd::NT) void bwd_flag(long long* __restrict__ hacc, const int* __restrict__ ycur,
                                                const void* __restrict__ xcur, const float* P, const uint16_t* w1bf,
                                                const uint16_t* __restrict__ pooled,
                                                const uint8_t* __restrict__ code, int phint,
                                                const float* __restrict__ Gr, Ctrl* __restrict__ ctrl,
                                                const void* __restrict__ X, const int* __restrict__ labels,
                                                float* __restrict__ G, long long* __restrict__ hconv, float* Pw,
                                                float* Vw, uint16_t* w1bf_out, unsigned long long* st,
                                                void* __restrict__ xnext, long long* __restrict__ xtag) {
  bwd_body<U8, true, CfgFlagBwd>(hacc, ycur, xcur, phint, 0, P, w1bf, pooled, code, ctrl, X, labels, G, hconv, 1, Pw,
                                 Vw, w1bf_out, st, Gr, XArgs{}, xnext, xtag, 0);
}

// =================================================================================
// flush: apply the pending (deferred) update to every parameter, zero the gradient
// buffers, fold the pending metrics into the epoch accumulators, clear `pending`.
// =================================================================================
// G / hconv: the reduced gradient (the peer all-reduce's `out` when it is folded into the
// step, see ConvNetBuffers::Gr); hconv_w: the buffer bwd adds into (both parities cleared)
__global__ __launch_bounds__(1024) void flush(float* __restrict__ P, float* __restrict__ G, float* __restrict__ V,
                                             const float* __restrict__ W1alt, const float* __restrict__ V1alt,
                                             long long* __restrict__ hconv, const float* __restrict__ calt,
                                             long long* __restrict__ hacc, int B, int eager,
                                             uint16_t* __restrict__ w1bf, Ctrl* __restrict__ ctrl,
                                             long long* __restrict__ hconv_w, int phint) {
  // w1bf: buffer 0 of the bf16 copy -- the live one from here on (the parity returns to 0).
  // Eager: nothing here writes it; w1bf_live0 ran first unless the host knew the parity to be 0
  const Ctrl c = *ctrl;
  if (phint >= 0 && phint != c.wpar && blockIdx.x == 0 && threadIdx.x == 0)  // (as in the step kernels)
    __hip_atomic_fetch_or(&ctrl->bad, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool mom = c.momentum != 0.f, pend = c.pending != 0;
  // after a step's bwd: current W1 / conv parameters live in the alternates when wpar is
  // set; the pending conv gradient is in hconv[wpar ^ 1]
  const long long* hg = hconv + (c.wpar ^ 1) * NCONV;
  // eager: W1 is current and its gradient was never stored -- only the conv and
  // b1/W2/b2 parameters are visited
  const int nvisit = eager ? NPARAM - (OFF_B1 - OFF_W1) : NPARAM;
  for (int iv = blockIdx.x * blockDim.x + threadIdx.x; iv < nvisit; iv += gridDim.x * blockDim.x) {
    const int i = eager && iv >= OFF_W1 ? iv + (OFF_B1 - OFF_W1) : iv;
    const bool w1 = i >= OFF_W1 && i < OFF_B1;
    const bool alt1 = !eager && c.wpar && w1, altc = c.wpar && i < NCONV;
    const float w = alt1 ? W1alt[i - OFF_W1] : (altc ? calt[i] : P[i]);
    const float v = alt1 ? V1alt[i - OFF_W1] : (altc ? calt[NCONV + i] : V[i]);
    const float g = i < NCONV ? from_fix(hg[i], CINV) : G[i];
    float wn, vn;
    sgd_or_keep(pend && !(eager && w1), w, g, v, c, wn, vn);  // eager: W1 is already current
    P[i] = wn;
    if (mom) V[i] = vn;
    if (w1) w1bf[i - OFF_W1] = f2bf(wn);
  }
  // the fixed-point accumulators start the next step at zero -- except the conv-gradient
  // parity read above (hg): other threads / blocks of THIS launch may not have loaded it
  // yet, and zeroing it here raced with them (a lost conv gradient on one rank, seen as
  // replicas whose conv parameters differed after an epoch flush).  That parity needs no
  // zero: after the flush nothing pending reads it, and the step that next writes it
  // zeroes it first (fwd's owner block).
  const int rp = c.wpar ^ 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * NCONV + 2 * B * HID; i += gridDim.x * blockDim.x) {
    if (i < 2 * NCONV) {
      const bool read_parity = i / NCONV == rp;
      if (!read_parity) hconv[i] = 0;
      if (!read_parity || hconv_w != hconv) hconv_w[i] = 0;
    } else {
      const int j = i - 2 * NCONV;  // (row j / HID of both parities, column j % HID)
      hacc[(j >> 6) * HACC_PITCH + (j & 63)] = 0;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && pend) {
    ctrl->acc_loss = c.acc_loss + G[OFF_LOSS];
    ctrl->acc_correct = c.acc_correct + G[OFF_CORR];
    ctrl->acc_count = c.acc_count + G[OFF_CNT];
    // the metric tail is folded: the next bwd's fold of "the previous step's metric" (world 1
    // / the standalone all-reduce) must add nothing (the gradient itself is never re-read:
    // the next fwd applies no update)
    G[OFF_LOSS] = G[OFF_CORR] = G[OFF_CNT] = 0.f;
  }
  __syncthreads();
  // one block (eager world 1: 1,034 parameters): every read of the ctrl block is behind the
  // barrier above, so no arrival ticket (a returning atomic costs the kernel ~1.5 us)
  if (threadIdx.x == 0) {
    if (gridDim.x == 1 ||
        __hip_atomic_fetch_add(&ctrl->flush_ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
            (int)gridDim.x - 1) {
      ctrl->wpar = 0;
      ctrl->pending = 0;
      ctrl->flush_ticket = 0;
      ctrl->ticket = 0;  // (the sharded bwd's arrival count: bounded between flushes)
    }
  }
}

// Eager update, ahead of flush: the live bf16 W1 buffer is the ctrl block's parity; flush
// returns the parity to 0, so after an odd number of steps buffer 1 is copied over buffer 0
// (nothing to do at parity 0: the launch is skipped when the host knows that).  16 bytes per
// thread, FEAT * HID / 8 units.
__global__ __launch_bounds__(512) void w1bf_live0(const Ctrl* __restrict__ ctrl, const uint4* __restrict__ b1,
                                                  uint4* __restrict__ b0) {
  if (ctrl->wpar == 0) return;
  const int i = blockIdx.x * 512 + threadIdx.x;
  if (i < FEAT * HID / 8) b0[i] = b1[i];
}

// =================================================================================
// sharded step: the pending update's reduced gradient gathered for flush / the host
// (waits for every unit and every rank's small message of the last exchange epoch, then
// writes the small sums into the gradient staging's b1 / W2 / b2 / metric slots and the
// conv sum into hred[wpar ^ 1], where flush reads them).  One block; nothing pending: no-op.
// It depends only on every rank having run that step's bwd -- not on their calling it.
// =================================================================================
__global__ __launch_bounds__(512) void sh_gather(Ctrl* __restrict__ ctrl, const XArgs xa, long long* __restrict__ hred,
                                                 int NS, int PP) {
  const Ctrl c = *ctrl;
  if (!c.pending) return;
  const unsigned xe = (unsigned)c.xcnt;
  const int ps = xe & 1, NU = 4 * NS, tid = threadIdx.x;
  float* xo = xa.out[xa.rank];
  // every block: its units (u = block, block + grid, ...); bf16 exchange: expanded into the
  // fp32 staging that flush reads
  for (int u = blockIdx.x; u < NU; u += gridDim.x) {
    if (tid < 2) x_wait(xa, x_gflag(xo, NU, u, tid), xe, XW_UNIT);
    __syncthreads();
    if (xa.gbf16) {
      const int sl = u >> 2, q = u & 3, k0 = sl * PP * 32, k1 = min(FEAT, k0 + PP * 32);
      const uint16_t* g16 = reinterpret_cast<const uint16_t*>(xo + kXG16);
      for (int e = tid; e < (k1 - k0) * 16; e += 512) {
        const long idx = (long)(k0 + (e >> 4)) * HID + 16 * q + (e & 15);
        xo[kXGred + OFF_W1 + idx] = bf2f(g16[idx]);
      }
    }
  }
  if (blockIdx.x != 0) return;
  if (tid < xa.world) x_wait(xa, x_sflag(xo, NU, ps, tid), xe, XW_SMALL);
  __syncthreads();
  for (int i = tid; i < NSMALL + 3; i += 512) {
    float a = 0.f;
    for (int r = 0; r < xa.world; ++r) a += x_small(xo, ps, r)[SM_GRAD + i];
    xo[kXGred + (i < NSMALL ? OFF_B1 + i : OFF_LOSS + i - NSMALL)] = a;
  }
  for (int i = tid; i < NCONV; i += 512) {
    long long q = 0;
    for (int r = 0; r < xa.world; ++r) q += reinterpret_cast<const long long*>(x_small(xo, ps, r) + SM_CONV)[i];
    hred[(c.wpar ^ 1) * NCONV + i] = q;
  }
}

}  // namespace convnet2

// ---------------------------------------------------------------------------------
// Host-side launchers (no allocation / sync: capturable into a hipGraph).
// ---------------------------------------------------------------------------------
int convnet_num_slices(int PP) { return (convnet::NPOS + PP - 1) / PP; }
// int64 elements of the dense-1 accumulator (both parities, rows HACC_PITCH apart)
long convnet_hacc_elems(int B) { return 2L * B * convnet::HACC_PITCH; }
size_t convnet_grad_count(int) { return (size_t)convnet::NGRAD; }
// fwd images per block = 2^lg: 16 up to B = 256 (more blocks, shorter per-block chains),
// 64 beyond (bounded replication of the W1-slice / conv-parameter loads)
int convnet_f1_lg(int B) { return B <= 256 ? 4 : 6; }

size_t convnet2_fwd_lds(int PP, int lg) {
  using namespace convnet;
  const int KP = kpitch(PP), IB = 1 << lg;
  const size_t xsb = (size_t)IB * XR * IMG * 4, partb = (size_t)IB * HID * 4;
  return (xsb > partb ? xsb : partb) + (size_t)(IB + HID) * KP * 2 + CONV_LDS_BYTES + (size_t)IB * PP * 32 + 256 * 4;
}
// flagship: the layout of bwd_flag (CfgFlagBwd::AUX: dps in a region of its own behind the head
// scratch instead of aliasing it)
// LDS bytes one role of the flagship backward needs (CfgFlagBwd::SPLIT; role 0 conv, 1 W1):
// the layouts of bwd_body
//   conv role  head | xs | dps | dhs | w1s | cs | red   (cs: a byte per code, or the conv
//              gradient's pre-decoded entries, CfgFlagBwd::CGPRE)
//   W1 role    head | pt | dht | ared (one float per aux thread)
static size_t bwd_flag_code_bytes(int PP) {
  return (size_t)convnet::CH * PP * 32 * (convnet2::CfgFlagBwd::CGPRE ? convnet::CGE_BYTES : 1);
}
size_t convnet2_bwd_role_lds(int PP, int role) {
  using namespace convnet;
  const size_t head = (size_t)convnet2::HEAD_BYTES, tile = (size_t)PP * 32 * HP * 2, slack = 16 + 256 * 4;
  if (role == 0)
    return head + XS_BYTES + (size_t)CH * (PP * 32 + 4) * 4 + (size_t)2 * CH * HP * 2 + tile + bwd_flag_code_bytes(PP) +
           (size_t)16 * NCONV * 4 + slack;
  return head + tile + (size_t)2 * HID * HP * 2 + (size_t)512 * 4 + slack;
}
int convnet2_bwd_flag_blocks() { return convnet2::CfgFlagBwd::GRID; }
int convnet2_bwd_flag_split() { return convnet2::CfgFlagBwd::SPLIT; }

size_t convnet2_bwd_lds(int PP, bool flagship) {
  using namespace convnet;
  if (flagship && convnet2::CfgFlagBwd::SPLIT != 0) {  // one launch: the larger of the two roles
    const size_t a = convnet2_bwd_role_lds(PP, 0), b = convnet2_bwd_role_lds(PP, 1);
    return a > b ? a : b;
  }
  const int KD = PP * 32 + 4;
  const size_t dpsb = (size_t)CH * KD * 4;
  const size_t rb = flagship && convnet2::CfgFlagBwd::AUX != 0 ? (size_t)convnet2::HEAD_BYTES + dpsb
                    : dpsb > (size_t)convnet2::HEAD_BYTES     ? dpsb
                                                               : (size_t)convnet2::HEAD_BYTES;
  const size_t redb = (size_t)16 * NCONV * 4;  // `red` spans pt + dht after the MFMAs
  const size_t ptdht = (size_t)PP * 32 * HP * 2 + (size_t)2 * HID * HP * 2;
  return XS_BYTES + rb + (ptdht > redb ? ptdht : redb) + (size_t)2 * CH * HP * 2 + (size_t)PP * 32 * HP * 2 +
         (flagship ? bwd_flag_code_bytes(PP) : (size_t)CH * PP * 32) + 16 + 256 * 4;
}

// eager W1 update: world-1 runs with the single-chunk backward (B <= 64) only
static int eager2(const ConvNetBuffers& b, int B) { return b.eager_w1 && B <= convnet::CH ? 1 : 0; }

static XArgs xargs(const ConvNetBuffers& b) {
  if (b.xa) return *b.xa;
  XArgs a{};
  return a;  // world 0: not sharded
}

static int ppb_of(const ConvNetBuffers& b, int PP) { return b.ppb > 0 ? b.ppb : PP; }

// The constant-configuration kernels (fwd_flag / bwd_flag) run the step exactly when BOTH
// launches have the flagship configuration: world 1 (no exchange, no folded all-reduce
// staging), 64 images, the default slicing of either kernel, eager W1 update -- and the
// switch is on.  Anything else runs the generic kernels.
bool convnet2_specialised(const ConvNetBuffers& b, int B, int PP) {
  using namespace convnet;
  using namespace convnet2;
  // (a role per block: the conv block of a slice reads the bf16 W1 slice its W1 block rewrites,
  // so the two parity buffers of the copy must be distinct)
  const bool two = b.w1bf_alt != nullptr && b.w1bf_alt != b.w1bf;
  return !b.force_generic && !b.xa && !b.Gr && !b.hconv_r && B == CH && PP == CfgFlagFwd::PP &&
         convnet_f1_lg(B) == CfgFlagFwd::LG && ppb_of(b, PP) == CfgFlagBwd::PP && eager2(b, B) == 1 &&
         (two || CfgFlagBwd::SPLIT == 0);
}

// The bf16 W1 copy as the step kernels take it (see CfgFlagBwd): (live, other) by the parity
// hint, or (buffer 0, buffer 1) when the host does not know the parity.  One buffer only
// (w1bf_alt null): both are that buffer -- the in-place copy of one block per slice.
struct W1bfPair {
  uint16_t* live;
  uint16_t* other;
};
static W1bfPair w1bf_pair(const ConvNetBuffers& b) {
  uint16_t* alt = b.w1bf_alt ? b.w1bf_alt : b.w1bf;
  return b.par_hint == 1 ? W1bfPair{alt, b.w1bf} : W1bfPair{b.w1bf, alt};
}

template <bool U8>
static void launch2_fwd(const ConvNetBuffers& b, int B, int PP, hipStream_t st) {
  using namespace convnet;
  const int NS = convnet_num_slices(PP);
  const int lg = convnet_f1_lg(B);
  const dim3 g1(NS, (B + (1 << lg) - 1) >> lg);
  const W1bfPair w1 = w1bf_pair(b);
  if (convnet2_specialised(b, B, PP)) {
    hipLaunchKernelGGL((convnet2::fwd_flag<U8>), g1, dim3(convnet2::CfgFlagFwd::NT), convnet2_fwd_lds(PP, lg), st,
                       b.xnext, b.xtag, w1.live, b.P, b.V, b.calt, b.hconv, b.G, b.ctrl, b.X, b.pooled, b.code, b.hacc,
                       b.hconv, b.stamps, b.labels, b.xcur, b.ycur, b.par_hint, w1.other);
    return;
  }
  hipLaunchKernelGGL((convnet2::fwd<U8>), g1, dim3(512), convnet2_fwd_lds(PP, lg), st,
                     B <= CH ? b.xnext : nullptr, w1.live, b.P, b.V, b.calt, b.hconv_r ? b.hconv_r : b.hconv,
                     b.Gr ? b.Gr : b.G, B | (PP << 16), lg | (eager2(b, B) << 8), b.ctrl, b.X, b.W1alt, b.V1alt,
                     b.pooled, b.code, b.hacc, b.hconv, b.stamps, xargs(b), b.xtag, b.labels,
                     B <= CH ? b.xcur : nullptr, b.ycur, b.par_hint, w1.other);
}

template <bool U8>
static void launch2_bwd(const ConvNetBuffers& b, int B, int PPf, hipStream_t st) {
  using namespace convnet;
  const int PP = ppb_of(b, PPf);
  const int NS = convnet_num_slices(PP);
  // aux elements (b1/W2/b2 gradients + metric tail) per block, and a power-of-two thread
  // count per element (<= 64) that fits them in 512 threads
  const int auxm = convnet2::aux_split(NS);
  const W1bfPair w1 = w1bf_pair(b);
  if (convnet2_specialised(b, B, PPf))
    hipLaunchKernelGGL((convnet2::bwd_flag<U8>), dim3(convnet2::CfgFlagBwd::GRID), dim3(convnet2::CfgFlagBwd::NT), convnet2_bwd_lds(PP, true), st, b.hacc, b.ycur, b.xcur,
                       b.P, w1.live, b.pooled, b.code, b.par_hint, b.G, b.ctrl, b.X, b.labels, b.G, b.hconv, b.P, b.V,
                       w1.other, b.stamps ? b.stamps + 2 * 256 * 16 : nullptr, b.xnext, b.xtag);
  else if (B <= CH)
    hipLaunchKernelGGL((convnet2::bwd<U8, true>), dim3(NS), dim3(512), convnet2_bwd_lds(PP), st, b.hacc,
                       B <= CH ? b.ycur : nullptr, B <= CH ? b.xcur : nullptr, b.par_hint, B | (PP << 16), b.P,
                       w1.live, b.pooled, b.code, b.ctrl, b.X, b.labels, b.G, b.hconv, eager2(b, B), b.P, b.V, w1.other,
                       b.stamps ? b.stamps + 2 * 256 * 16 : nullptr, b.Gr ? b.Gr : b.G, xargs(b), b.xnext, b.xtag,
                       auxm);
  else
    hipLaunchKernelGGL((convnet2::bwd<U8, false>), dim3(NS), dim3(512), convnet2_bwd_lds(PP), st, b.hacc,
                       B <= CH ? b.ycur : nullptr, B <= CH ? b.xcur : nullptr, b.par_hint, B | (PP << 16), b.P,
                       w1.live, b.pooled, b.code, b.ctrl, b.X, b.labels, b.G, b.hconv, eager2(b, B), b.P, b.V, w1.other,
                       b.stamps ? b.stamps + 2 * 256 * 16 : nullptr, b.Gr ? b.Gr : b.G, xargs(b), b.xnext, b.xtag,
                       auxm);
}

int convnet2_fwd_threads(const ConvNetBuffers& b, int B, int PP) {
  return convnet2_specialised(b, B, PP) ? convnet2::CfgFlagFwd::NT : 512;
}

hipError_t convnet2_fwd_compiled_threads(const ConvNetBuffers& b, int B, int PP, int* out) {
  const void* f = convnet2_specialised(b, B, PP)
                      ? (b.x_u8 ? (const void*)convnet2::fwd_flag<true> : (const void*)convnet2::fwd_flag<false>)
                      : (b.x_u8 ? (const void*)convnet2::fwd<true> : (const void*)convnet2::fwd<false>);
  hipFuncAttributes at;
  const hipError_t e = hipFuncGetAttributes(&at, f);
  if (e == hipSuccess) *out = at.maxThreadsPerBlock;
  return e;
}

int convnet2_bwd_blocks(const ConvNetBuffers& b, int B, int PP) {
  return convnet2_specialised(b, B, PP) ? convnet2::CfgFlagBwd::GRID : convnet_num_slices(ppb_of(b, PP));
}

int convnet2_bwd_threads(const ConvNetBuffers& b, int B, int PP) {
  return convnet2_specialised(b, B, PP) ? convnet2::CfgFlagBwd::NT : 512;
}

hipError_t convnet2_bwd_compiled_threads(const ConvNetBuffers& b, int B, int PP, int* out) {
  const void* f = convnet2_specialised(b, B, PP)
                      ? (b.x_u8 ? (const void*)convnet2::bwd_flag<true> : (const void*)convnet2::bwd_flag<false>)
                  : B <= convnet::CH
                      ? (b.x_u8 ? (const void*)convnet2::bwd<true, true> : (const void*)convnet2::bwd<false, true>)
                      : (b.x_u8 ? (const void*)convnet2::bwd<true, false> : (const void*)convnet2::bwd<false, false>);
  hipFuncAttributes at;
  const hipError_t e = hipFuncGetAttributes(&at, f);
  if (e == hipSuccess) *out = at.maxThreadsPerBlock;
  return e;
}

hipError_t convnet2_launch_fwd(const ConvNetBuffers& b, int B, int PP, hipStream_t st) {
  if (!b.hacc || !b.hconv || !b.calt || B > 0xffff) return hipErrorInvalidValue;
  if (b.x_u8) launch2_fwd<true>(b, B, PP, st);
  else launch2_fwd<false>(b, B, PP, st);
  return hipGetLastError();
}

hipError_t convnet2_launch_bwd(const ConvNetBuffers& b, int B, int PP, hipStream_t st) {
  if (!b.hacc || !b.hconv || !b.calt || B > 0xffff) return hipErrorInvalidValue;
  if (convnet2_bwd_lds(ppb_of(b, PP), convnet2_specialised(b, B, PP)) > 160 * 1024) return hipErrorInvalidValue;
  if (b.xa && b.xa->ppb != ppb_of(b, PP)) return hipErrorInvalidValue;
  if (b.x_u8) launch2_bwd<true>(b, B, PP, st);
  else launch2_bwd<false>(b, B, PP, st);
  return hipGetLastError();
}

hipError_t convnet2_launch_step(const ConvNetBuffers& b, int B, int PP, hipStream_t st) {
  hipError_t e = convnet2_launch_fwd(b, B, PP, st);
  return e != hipSuccess ? e : convnet2_launch_bwd(b, B, PP, st);
}

hipError_t convnet2_launch_gather(const ConvNetBuffers& b, int PP, hipStream_t st) {
  if (!b.xa || b.xa->world < 2 || !b.hconv_r) return hipErrorInvalidValue;
  const int ppb = ppb_of(b, PP);
  hipLaunchKernelGGL(convnet2::sh_gather, dim3(57), dim3(512), 0, st, b.ctrl, *b.xa, b.hconv_r, convnet_num_slices(ppb),
                     ppb);
  return hipGetLastError();
}

hipError_t convnet2_launch_flush(const ConvNetBuffers& b, int B, hipStream_t st) {
  // eager: buffer 0 of the bf16 W1 copy becomes the live one (flush returns the parity to 0)
  if (eager2(b, B) && b.w1bf_alt && b.w1bf_alt != b.w1bf && b.par_hint != 0)
    hipLaunchKernelGGL(convnet2::w1bf_live0, dim3((convnet::FEAT * convnet::HID / 8 + 511) / 512), dim3(512), 0, st, b.ctrl,
                       reinterpret_cast<const uint4*>(b.w1bf_alt), reinterpret_cast<uint4*>(b.w1bf));
  hipLaunchKernelGGL(convnet2::flush, dim3(eager2(b, B) ? 1 : 340), dim3(eager2(b, B) ? 1024 : 256), 0, st, b.P, b.Gr ? b.Gr : b.G, b.V,
                     b.W1alt, b.V1alt, b.hconv_r ? b.hconv_r : b.hconv, b.calt, b.hacc, B, eager2(b, B), b.w1bf, b.ctrl,
                     b.hconv, b.par_hint);
  return hipGetLastError();
}

hipError_t convnet2_set_lds_limits() {
  const void* fns[10] = {(const void*)convnet2::fwd<false>,        (const void*)convnet2::fwd<true>,
                         (const void*)convnet2::bwd<false, true>,  (const void*)convnet2::bwd<true, true>,
                         (const void*)convnet2::bwd<false, false>, (const void*)convnet2::bwd<true, false>,
                         (const void*)convnet2::fwd_flag<false>,   (const void*)convnet2::fwd_flag<true>,
                         (const void*)convnet2::bwd_flag<false>,   (const void*)convnet2::bwd_flag<true>};
  for (const void* f : fns) {
    hipFuncAttributes at;
    hipError_t e = hipFuncGetAttributes(&at, f);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - (int)at.sharedSizeBytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace damd
