// Device-side building blocks shared by the per-layer kernel files of the generic path
// (csrc/kernels/bn.hip, pool.hip, loss_head.hip, optimizer.hip, glue.hip): the 8-channel
// bf16 vector helpers, the launch-grid helper, the in-consumer BatchNorm finalize prologues
// and the wave sum of the fixed-order reductions.  A helper used by one file only lives in
// that file.
//
// Layout: NHWC bf16 activations, channel count C % 8 == 0, so every thread moves one
// 16-byte vector of 8 channels (global_load_dwordx4) and keeps the 8 per-channel
// parameters in registers.
#pragma once
#include "bn_fin.h"
#include "damd_common.h"
#include "layer_ops.h"

namespace damd {

constexpr int NT = 256;

__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ uint4 pack8(const float* f) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f2bf(f[2 * i]) | ((uint32_t)f2bf(f[2 * i + 1]) << 16);
  return uint4{w[0], w[1], w[2], w[3]};
}
__device__ __forceinline__ void ld8f(const float* p, float* f) {
  float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

inline int grid_for(long work, int per_block = NT, int cap = 8192) {
  long g = (work + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

// the sum of v over the 64 lanes of a wave, in every lane (fixed shuffle tree); SX_NW waves
// per block meet in LDS
constexpr int SX_NW = NT / 64;
__device__ __forceinline__ float sx_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// ---- BatchNorm -------------------------------------------------------------------------
// relu(BN(x)) rounded to bf16 exactly as bn_apply stores it: ReLU masks recomputed from
// the BN input (relu_mask == 2 in bn.hip, the stem kernels of pool.hip) equal those of the
// stored output.
__device__ __forceinline__ void bn_relu8(const float* x, const float* sc, const float* sh, float* y) {
#pragma unroll
  for (int e = 0; e < 8; ++e) y[e] = bf2f(f2bf(fmaxf(fmaf(x[e], sc[e], sh[e]), 0.f)));
}

// ---- in-consumer finalize (BNFin / BNBwdFin, layer_ops.h) ----------------------------
// Every block derives the per-channel coefficients of all C channels from the fixed-point
// accumulators into LDS (s: [4][C] for the forward, [3][C] for the backward); block 0 also
// publishes them (st / co), updates the moving statistics and adds dgamma / dbeta.  The
// returned pointer replaces st / co in the kernel body (global when acc is null).
// backward coefficients of channel c: dx = a dz + b + cc xhat; pub: co, dgamma, dbeta
__device__ __forceinline__ void bn_bwd_fin_sums(const BNBwdFin& f, int C, int c, double s, double q,
                                                const float* st, bool pub, float& a, float& b, float& cc) {
  const float db = (float)s, dg = (float)q;
  a = st[2 * C + c];
  b = -a * db / f.count;
  cc = -a * dg / f.count;
  if (pub) {
    if (f.dbeta) f.dbeta[c] += db;
    if (f.dgamma) f.dgamma[c] += dg;
    f.co[c] = a;
    f.co[C + c] = b;
    f.co[2 * C + c] = cc;
  }
}
__device__ __forceinline__ const float* bn_fin_prologue(const BNFin& f, int C, float* s, const float* st) {
  if (f.acc == nullptr) return st;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    double a, b;
    acc_sums(f.acc, f.reps, C, c, a, b);
    bn_fin_sums(f, C, c, a, b, blockIdx.x == 0, s[c], s[C + c], s[2 * C + c], s[3 * C + c]);
  }
  __syncthreads();
  return s;
}
__device__ __forceinline__ const float* bn_bwd_fin_prologue(const BNBwdFin& f, int C, const float* st, float* s,
                                                            const float* co) {
  if (f.acc == nullptr) return co;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    double a, b;
    acc_sums2(f.acc, f.reps, C, c, a, b);
    bn_bwd_fin_sums(f, C, c, a, b, st, blockIdx.x == 0, s[c], s[C + c], s[2 * C + c]);
  }
  __syncthreads();
  return s;
}
// per-block (fp32, fixed order) partial of channel ch -> replica blockIdx.x % reps of the
// accumulator (order-independent fixed point), or the partials row of this block
__device__ __forceinline__ void put_partial(float* part, long long* acc, int reps, int C, int ch, float a, float b) {
  if (acc) {
    long long* r = acc + (size_t)(blockIdx.x % reps) * 4 * C;  // (backward sums: hi / lo planes)
    long long* flag = acc + (size_t)max(reps, 1) * 4 * C + ch;   // sticky plane
    bnacc_add2(r + ch, r + C + ch, flag, a);
    bnacc_add2(r + 2 * C + ch, r + 3 * C + ch, flag, b);
  } else {
    part[(size_t)blockIdx.x * 2 * C + ch] = a;
    part[(size_t)blockIdx.x * 2 * C + C + ch] = b;
  }
}

// blocks of a consumer that finalizes in its prologue: every block pays one pass over the
// C channels, so the grid-stride kernels run at most 8 blocks per CU
constexpr int FIN_GRID_CAP = 2048;
constexpr int FIN_MAX_C = 4096;
static const BNFin kNoFin{};
static const BNBwdFin kNoBwdFin{};

}  // namespace damd
