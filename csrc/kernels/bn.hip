// BatchNorm of the generic path: training forward (apply with fused residual add + ReLU),
// backward (reduce / apply, single and dual), the stand-alone finalize kernels over fp32
// partials, and the inference st rows from the moving statistics.
//
// Statistics are reduced in fp32 per block (LDS, fixed order).  Across blocks they either go
// through partials [T][2][C] summed in fp64 by a finalize launch (bn_finalize /
// bn_bwd_finalize), or -- the engines' path -- into int64 fixed-point accumulators by integer
// atomics (order independent, damd_common.h bnacc_*), which the consumer kernel decodes in
// its prologue (layer_dev.h bn_fin_prologue / bn_bwd_fin_prologue): no finalize launch.
// The launch heuristics at the end of the kernels balance that prologue against the grid.
#include <cstdlib>

#include "layer_dev.h"

namespace damd {
namespace {

// Sum the partials [T][2][C] over T in fp64 for the 8 channels c0..c0+7 of this block
// (FT = 1024 threads).  Thread t owns value v = t % 16 of the 16-value record (8 sums, 8
// second statistics) and rows t / 16 + 64 k: 64 row slices with up to 16 loads each in
// flight, so the ResNet-18 partial counts (T = 784..1024; 3136 at the stem) take one
// batch of loads (four with the 256-thread version: ~1 us of latency each), then a
// three-level LDS tree (64 -> 16 -> 1 slices, fixed order: deterministic).
// On return sums[j] (j < 8) is the channel sum, sums[8 + j] the second statistic.
constexpr int FT = 1024, FSL = FT / 16;
__device__ __forceinline__ void reduce_partials8(const float* __restrict__ part, int T, int C, int c0,
                                                 double* sums) {
  __shared__ double red[FSL][17];
  __shared__ double red2[16][17];
  const int t = threadIdx.x, v = t & 15, sl = t >> 4;
  const float* p = part + (v < 8 ? c0 + v : C + c0 + (v - 8));
  const size_t row = (size_t)2 * C;
  double a = 0.0;
  for (int i0 = sl; i0 < T; i0 += FSL * 16) {
    float f[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int i = i0 + FSL * u;
      f[u] = p[(size_t)min(i, T - 1) * row];
      f[u] = i < T ? f[u] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) a += (double)f[u];
  }
  red[sl][v] = a;
  __syncthreads();
  if (t < 256) {
    const int g = t >> 4;
    double b = 0.0;
#pragma unroll
    for (int q = 0; q < FSL / 16; ++q) b += red[g * (FSL / 16) + q][v];
    red2[g][v] = b;
  }
  __syncthreads();
  if (t < 16) {
    double s2 = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) s2 += red2[q][t];
    sums[t] = s2;
  }
  __syncthreads();
}

__global__ __launch_bounds__(FT) void bn_finalize_k(const float* part, int T, int C, float count,
                                                    const float* gamma, const float* beta, float eps, float mom,
                                                    float* rmean, float* rvar, float* st) {
  __shared__ double sums[16];
  const int c0 = blockIdx.x * 8;
  reduce_partials8(part, T, C, c0, sums);
  if (threadIdx.x >= 8) return;
  const int c = c0 + threadIdx.x;
  const double mean = sums[threadIdx.x] / count;
  double var = fma(-mean, mean, sums[8 + threadIdx.x] / count);  // (explicit fmas: as bn_fin.h)
  if (var < 0.0) var = 0.0;
  const float m = (float)mean, v = (float)var;
  const float inv = rsqrtf(v + eps);
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  const float sc = g * inv;
  st[c] = m;
  st[C + c] = inv;
  st[2 * C + c] = sc;
  st[3 * C + c] = fmaf(-m, sc, b);
  if (rmean) {
    rmean[c] = fmaf(rmean[c], mom, m * (1.f - mom));
    rvar[c] = fmaf(rvar[c], mom, v * (1.f - mom));
  }
}

__global__ __launch_bounds__(NT) void bn_apply_k(const uint16_t* __restrict__ x, const float* st_in,
                                                 const uint16_t* __restrict__ r, const float* st2_in,
                                                 int res_mode, int relu, uint16_t* __restrict__ y, long n8, int C,
                                                 BNFin f1, BNFin f2) {
  extern __shared__ float sfin[];  // [4][C] (f1), then [4][C] (f2)
  const float* st = bn_fin_prologue(f1, C, sfin, st_in);
  const float* st2 = res_mode == 2 ? bn_fin_prologue(f2, C, sfin + 4 * C, st2_in) : st2_in;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += (long)gridDim.x * NT) {
    const int c = (int)((i * 8) % C);
    float xv[8], sc[8], sh[8];
    unpack8(reinterpret_cast<const uint4*>(x)[i], xv);
    ld8f(st + 2 * C + c, sc);
    ld8f(st + 3 * C + c, sh);
#pragma unroll
    for (int e = 0; e < 8; ++e) xv[e] = fmaf(xv[e], sc[e], sh[e]);
    if (res_mode) {
      float rv[8];
      unpack8(reinterpret_cast<const uint4*>(r)[i], rv);
      if (res_mode == 2) {
        float sc2[8], sh2[8];
        ld8f(st2 + 2 * C + c, sc2);
        ld8f(st2 + 3 * C + c, sh2);
#pragma unroll
        for (int e = 0; e < 8; ++e) rv[e] = rv[e] * sc2[e] + sh2[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[e] += rv[e];
    }
    if (relu) {
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[e] = fmaxf(xv[e], 0.f);
    }
    reinterpret_cast<uint4*>(y)[i] = pack8(xv);
  }
}

// Row-mapped apply kernels: thread t keeps channel group t % (C/8) for the whole launch,
// so its per-channel coefficients are loaded once into registers instead of once per
// 16-byte data vector (the flat kernels above fetched 2-7 coefficient vectors per data
// vector); BN_UNR rows per thread in flight.  Same arithmetic, bitwise equal output.
// Measured on ResNet-18: backward apply 9.9 -> 8.8 us per launch, forward apply unchanged
// (already at HBM rate); the same unrolling of bn_bwd_reduce_k's row loop was slower
// (8.6 -> 9.5 us) and is not used.  With the in-consumer finalize (BNFin / BNBwdFin) the
// first batch of rows is requested before the prologue, so the data fetch overlaps the
// accumulator read and the fp64 finalize instead of queueing behind them.
constexpr int BN_UNR = 4;
__global__ __launch_bounds__(NT) void bn_apply_rows_k(const uint16_t* __restrict__ x, const float* st,
                                                      const uint16_t* __restrict__ r, const float* st2,
                                                      int res_mode, int relu, uint16_t* __restrict__ y, long M, int C,
                                                      BNFin f1, BNFin f2) {
  extern __shared__ float sfin[];  // in-consumer finalize: [4][C] (f1), then [4][C] (f2)
  const int cg = C / 8, t = threadIdx.x, rpi = NT / cg;  // launcher: NT % cg == 0
  const int g = t % cg, rr = t / cg, c = g * 8;
  const long stride = (long)gridDim.x * rpi;
  const uint4* x4 = reinterpret_cast<const uint4*>(x);
  const uint4* r4 = reinterpret_cast<const uint4*>(r);
  uint4* y4 = reinterpret_cast<uint4*>(y);
  uint4 xq[BN_UNR], rq[BN_UNR];
  auto load = [&](long row0) {
#pragma unroll
    for (int u = 0; u < BN_UNR; ++u) {
      const long row = min(row0 + u * stride, M - 1);
      xq[u] = x4[row * cg + g];
      if (res_mode) rq[u] = r4[row * cg + g];
    }
  };
  long row0 = (long)blockIdx.x * rpi + rr;
  load(row0);
  st = bn_fin_prologue(f1, C, sfin, st);
  if (res_mode == 2) st2 = bn_fin_prologue(f2, C, sfin + 4 * C, st2);
  float sc[8], sh[8], sc2[8], sh2[8];
  ld8f(st + 2 * C + c, sc);
  ld8f(st + 3 * C + c, sh);
  if (res_mode == 2) {
    ld8f(st2 + 2 * C + c, sc2);
    ld8f(st2 + 3 * C + c, sh2);
  }
  for (bool first = true; row0 < M; row0 += stride * BN_UNR, first = false) {
    if (!first) load(row0);
#pragma unroll
    for (int u = 0; u < BN_UNR; ++u) {
      const long row = row0 + u * stride;
      if (row >= M) break;
      float xv[8];
      unpack8(xq[u], xv);
#pragma unroll
      for (int e = 0; e < 8; ++e) xv[e] = fmaf(xv[e], sc[e], sh[e]);
      if (res_mode) {
        float rv[8];
        unpack8(rq[u], rv);
        if (res_mode == 2) {
#pragma unroll
          for (int e = 0; e < 8; ++e) rv[e] = rv[e] * sc2[e] + sh2[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] += rv[e];
      }
      if (relu) {
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[e] = fmaxf(xv[e], 0.f);
      }
      y4[row * cg + g] = pack8(xv);
    }
  }
}

__global__ __launch_bounds__(NT) void bn_bwd_apply_rows_k(const uint16_t* __restrict__ dy,
                                                          const uint16_t* __restrict__ y, int relu_mask,
                                                          const uint16_t* __restrict__ x, const float* __restrict__ st,
                                                          const float* co, uint16_t* __restrict__ dx,
                                                          long M, int C, BNBwdFin bf) {
  extern __shared__ float sfin[];  // in-consumer finalize: [3][C]
  const int cg = C / 8, t = threadIdx.x, rpi = NT / cg;  // launcher: NT % cg == 0
  const int g = t % cg, rr = t / cg, c = g * 8;
  const long stride = (long)gridDim.x * rpi;
  const uint4* d4 = reinterpret_cast<const uint4*>(dy);
  const uint4* x4 = reinterpret_cast<const uint4*>(x);
  const uint4* y4 = reinterpret_cast<const uint4*>(y);
  uint4* o4 = reinterpret_cast<uint4*>(dx);
  uint4 dq[BN_UNR], xq[BN_UNR], yq[BN_UNR];
  auto load = [&](long row0) {
#pragma unroll
    for (int u = 0; u < BN_UNR; ++u) {
      const long row = min(row0 + u * stride, M - 1);
      dq[u] = d4[row * cg + g];
      xq[u] = x4[row * cg + g];
      if (relu_mask == 1) yq[u] = y4[row * cg + g];
    }
  };
  long row0 = (long)blockIdx.x * rpi + rr;
  load(row0);
  co = bn_bwd_fin_prologue(bf, C, st, sfin, co);
  float mean[8], inv[8], a[8], b[8], cc[8], sc[8], sh[8];
  ld8f(st + c, mean);
  ld8f(st + C + c, inv);
  ld8f(co + c, a);
  ld8f(co + C + c, b);
  ld8f(co + 2 * C + c, cc);
  if (relu_mask == 2) {
    ld8f(st + 2 * C + c, sc);
    ld8f(st + 3 * C + c, sh);
  }
  for (bool first = true; row0 < M; row0 += stride * BN_UNR, first = false) {
    if (!first) load(row0);
#pragma unroll
    for (int u = 0; u < BN_UNR; ++u) {
      const long row = row0 + u * stride;
      if (row >= M) break;
      float d[8], xv[8];
      unpack8(dq[u], d);
      unpack8(xq[u], xv);
      if (relu_mask) {
        float yv[8];
        if (relu_mask == 2)
          bn_relu8(xv, sc, sh, yv);
        else
          unpack8(yq[u], yv);
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] = yv[e] > 0.f ? d[e] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = a[e] * d[e] + b[e] + cc[e] * (xv[e] - mean[e]) * inv[e];
      o4[row * cg + g] = pack8(d);
    }
  }
}

// dz = dy * [y>0]; partial sums of dz and dz*xhat per channel for a contiguous row range.
// MODE = relu_mask (0 none, 1 mask from the stored y, 2 recomputed from x): a template
// argument, so the loads of RU rows (dy, x, y) are issued together before the first use --
// with the mask source behind a runtime branch and the dz stores (which may alias the next
// rows' loads) between rows, every row cost its own two memory round trips.  Rows are
// still accumulated in ascending order: the partials are bitwise those of the row loop.
constexpr int RED_RU = 4;
template <int MODE>
__global__ __launch_bounds__(NT) void bn_bwd_reduce_k(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
                                                      const uint16_t* __restrict__ x,
                                                      const float* __restrict__ st, uint16_t* __restrict__ dz_out,
                                                      float* __restrict__ part, long M, int C, long rows_per_block,
                                                      long long* __restrict__ acc, int reps, int rev) {
  __shared__ float red[2][NT * 8];
  const int cg = C / 8, t = threadIdx.x;
  const int rpi = NT / cg;  // rows per iteration
  const int g = t % cg, rr = t / cg;
  const int c = g * 8;
  // rev (tests, bn_reduce_reverse): block b reduces the rows of block G-1-b -- the same
  // partials, produced in a different order and added into different replicas
  const long blk = rev ? (long)gridDim.x - 1 - blockIdx.x : blockIdx.x;
  float s0[8], s1[8], mean[8], inv[8], sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s0[e] = s1[e] = 0.f;
  ld8f(st + c, mean);
  ld8f(st + C + c, inv);
  if (MODE == 2) {
    ld8f(st + 2 * C + c, sc);
    ld8f(st + 3 * C + c, sh);
  }
  const long r0 = blk * rows_per_block, r1 = min(M, r0 + rows_per_block);
  if (rr < rpi) {
    for (long row = r0 + rr; row < r1; row += (long)RED_RU * rpi) {
      uint4 dq[RED_RU], xq[RED_RU], yq[RED_RU];
#pragma unroll
      for (int u = 0; u < RED_RU; ++u) {
        const long off = (min(row + u * rpi, r1 - 1) * C + c) / 8;
        dq[u] = reinterpret_cast<const uint4*>(dy)[off];
        xq[u] = reinterpret_cast<const uint4*>(x)[off];
        if (MODE == 1) yq[u] = reinterpret_cast<const uint4*>(y)[off];
      }
#pragma unroll
      for (int u = 0; u < RED_RU; ++u) {
        const long rw = row + u * rpi;
        if (rw >= r1) break;
        const long off = (rw * C + c) / 8;
        float d[8], xv[8];
        unpack8(dq[u], d);
        unpack8(xq[u], xv);
        if (MODE) {
          float yv[8];
          if (MODE == 2)
            bn_relu8(xv, sc, sh, yv);
          else
            unpack8(yq[u], yv);
#pragma unroll
          for (int e = 0; e < 8; ++e) d[e] = yv[e] > 0.f ? d[e] : 0.f;
          if (dz_out) reinterpret_cast<uint4*>(dz_out)[off] = pack8(d);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          s0[e] += d[e];
          s1[e] += d[e] * (xv[e] - mean[e]) * inv[e];
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[0][t * 8 + e] = rr < rpi ? s0[e] : 0.f;
    red[1][t * 8 + e] = rr < rpi ? s1[e] : 0.f;
  }
  __syncthreads();
  // thread t < C sums channel t over the rpi row groups: element (rr*cg + g)*8 + e, c = 8g+e
  for (int ch = t; ch < C; ch += NT) {
    const int gg = ch / 8, e = ch % 8;
    float a = 0.f, b = 0.f;
    for (int q = 0; q < rpi; ++q) {
      a += red[0][(q * cg + gg) * 8 + e];
      b += red[1][(q * cg + gg) * 8 + e];
    }
    put_partial(part, acc, reps, C, ch, a, b);
  }
}

// Two BatchNorms fed by the same masked gradient (a ResNet downsampling block's output
// relu(BN2(x2) + BNd(xd))): ONE pass over dy and the mask source y for both -- per
// channel sum dz (shared), sum dz * xhat2, sum dz * xhatd -- each BN's partials into its own
// accumulator.  The row ranges, the per-thread order and the LDS tree are those of
// bn_bwd_reduce_k, so each accumulator receives bitwise the partials the single-BN launch
// would add (relu_mask 0 / 1 only; fixed-point accumulators only).
__global__ __launch_bounds__(NT) void bn_bwd_reduce2_k(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
                                                       int relu_mask, const uint16_t* __restrict__ x,
                                                       const uint16_t* __restrict__ x2, const float* __restrict__ st,
                                                       const float* __restrict__ st2, long M, int C,
                                                       long rows_per_block, long long* __restrict__ acc,
                                                       long long* __restrict__ acc2, int reps) {
  __shared__ float red[3][NT * 8];
  const int cg = C / 8, t = threadIdx.x;
  const int rpi = NT / cg;
  const int g = t % cg, rr = t / cg;
  const int c = g * 8;
  const long blk = blockIdx.x;
  float s0[8], s1[8], s2[8], mean[8], inv[8], mean2[8], inv2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s0[e] = s1[e] = s2[e] = 0.f;
  ld8f(st + c, mean);
  ld8f(st + C + c, inv);
  ld8f(st2 + c, mean2);
  ld8f(st2 + C + c, inv2);
  const long r0 = blk * rows_per_block, r1 = min(M, r0 + rows_per_block);
  if (rr < rpi) {
    for (long row = r0 + rr; row < r1; row += rpi) {
      const long off = (row * C + c) / 8;
      float d[8], xv[8], xw[8];
      unpack8(reinterpret_cast<const uint4*>(dy)[off], d);
      unpack8(reinterpret_cast<const uint4*>(x)[off], xv);
      unpack8(reinterpret_cast<const uint4*>(x2)[off], xw);
      if (relu_mask) {
        float yv[8];
        unpack8(reinterpret_cast<const uint4*>(y)[off], yv);
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] = yv[e] > 0.f ? d[e] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s0[e] += d[e];
        s1[e] += d[e] * (xv[e] - mean[e]) * inv[e];
        s2[e] += d[e] * (xw[e] - mean2[e]) * inv2[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[0][t * 8 + e] = rr < rpi ? s0[e] : 0.f;
    red[1][t * 8 + e] = rr < rpi ? s1[e] : 0.f;
    red[2][t * 8 + e] = rr < rpi ? s2[e] : 0.f;
  }
  __syncthreads();
  for (int ch = t; ch < C; ch += NT) {
    const int gg = ch / 8, e = ch % 8;
    float a = 0.f, b = 0.f, b2 = 0.f;
    for (int q = 0; q < rpi; ++q) {
      a += red[0][(q * cg + gg) * 8 + e];
      b += red[1][(q * cg + gg) * 8 + e];
      b2 += red[2][(q * cg + gg) * 8 + e];
    }
    put_partial(nullptr, acc, reps, C, ch, a, b);
    put_partial(nullptr, acc2, reps, C, ch, a, b2);
  }
}

// ... and the matching apply: both BNs' coefficients finalized in the prologue, dx and dx2
// from one read of dy / y (row mapping and arithmetic of bn_bwd_apply_rows_k)
__global__ __launch_bounds__(NT) void bn_bwd_apply2_rows_k(const uint16_t* __restrict__ dy,
                                                           const uint16_t* __restrict__ y, int relu_mask,
                                                           const uint16_t* __restrict__ x,
                                                           const uint16_t* __restrict__ x2,
                                                           const float* __restrict__ st,
                                                           const float* __restrict__ st2, uint16_t* __restrict__ dx,
                                                           uint16_t* __restrict__ dx2, long M, int C, BNBwdFin bf,
                                                           BNBwdFin bf2) {
  extern __shared__ float sfin[];  // [3][C] (bf), then [3][C] (bf2)
  const int cg = C / 8, t = threadIdx.x, rpi = NT / cg;
  const int g = t % cg, rr = t / cg, c = g * 8;
  const long stride = (long)gridDim.x * rpi;
  const uint4* d4 = reinterpret_cast<const uint4*>(dy);
  const uint4* x4 = reinterpret_cast<const uint4*>(x);
  const uint4* w4 = reinterpret_cast<const uint4*>(x2);
  const uint4* y4 = reinterpret_cast<const uint4*>(y);
  uint4* o4 = reinterpret_cast<uint4*>(dx);
  uint4* p4 = reinterpret_cast<uint4*>(dx2);
  uint4 dq[BN_UNR], xq[BN_UNR], wq[BN_UNR], yq[BN_UNR];
  auto load = [&](long row0) {
#pragma unroll
    for (int u = 0; u < BN_UNR; ++u) {
      const long row = min(row0 + u * stride, M - 1);
      dq[u] = d4[row * cg + g];
      xq[u] = x4[row * cg + g];
      wq[u] = w4[row * cg + g];
      if (relu_mask) yq[u] = y4[row * cg + g];
    }
  };
  long row0 = (long)blockIdx.x * rpi + rr;
  load(row0);
  const float* co = bn_bwd_fin_prologue(bf, C, st, sfin, bf.co);
  const float* co2 = bn_bwd_fin_prologue(bf2, C, st2, sfin + 3 * C, bf2.co);
  float mean[8], inv[8], a[8], b[8], cc[8], mean2[8], inv2[8], a2[8], b2[8], cc2[8];
  ld8f(st + c, mean);
  ld8f(st + C + c, inv);
  ld8f(co + c, a);
  ld8f(co + C + c, b);
  ld8f(co + 2 * C + c, cc);
  ld8f(st2 + c, mean2);
  ld8f(st2 + C + c, inv2);
  ld8f(co2 + c, a2);
  ld8f(co2 + C + c, b2);
  ld8f(co2 + 2 * C + c, cc2);
  for (bool first = true; row0 < M; row0 += stride * BN_UNR, first = false) {
    if (!first) load(row0);
#pragma unroll
    for (int u = 0; u < BN_UNR; ++u) {
      const long row = row0 + u * stride;
      if (row >= M) break;
      float d[8], xv[8], xw[8], o[8], p[8];
      unpack8(dq[u], d);
      unpack8(xq[u], xv);
      unpack8(wq[u], xw);
      if (relu_mask) {
        float yv[8];
        unpack8(yq[u], yv);
#pragma unroll
        for (int e = 0; e < 8; ++e) d[e] = yv[e] > 0.f ? d[e] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        o[e] = a[e] * d[e] + b[e] + cc[e] * (xv[e] - mean[e]) * inv[e];
        p[e] = a2[e] * d[e] + b2[e] + cc2[e] * (xw[e] - mean2[e]) * inv2[e];
      }
      o4[row * cg + g] = pack8(o);
      p4[row * cg + g] = pack8(p);
    }
  }
}

__global__ __launch_bounds__(FT) void bn_bwd_finalize_k(const float* part, int T, int C, float count,
                                                        const float* st, float* dgamma, float* dbeta, float* co) {
  __shared__ double sums[16];
  const int c0 = blockIdx.x * 8;
  reduce_partials8(part, T, C, c0, sums);
  if (threadIdx.x >= 8) return;
  const int c = c0 + threadIdx.x;
  const float db = (float)sums[threadIdx.x], dg = (float)sums[8 + threadIdx.x];
  if (dbeta) dbeta[c] += db;
  if (dgamma) dgamma[c] += dg;
  const float a = st[2 * C + c];
  co[c] = a;
  co[C + c] = -a * db / count;
  co[2 * C + c] = -a * dg / count;
}

__global__ __launch_bounds__(NT) void bn_bwd_apply_k(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y,
                                                     int relu_mask, const uint16_t* __restrict__ x,
                                                     const float* __restrict__ st, const float* co_in,
                                                     uint16_t* __restrict__ dx, long n8, int C, BNBwdFin bf) {
  extern __shared__ float sfin[];  // [3][C]
  const float* co = bn_bwd_fin_prologue(bf, C, st, sfin, co_in);
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += (long)gridDim.x * NT) {
    const int c = (int)((i * 8) % C);
    float d[8], xv[8], mean[8], inv[8], a[8], b[8], cc[8];
    unpack8(reinterpret_cast<const uint4*>(dy)[i], d);
    unpack8(reinterpret_cast<const uint4*>(x)[i], xv);
    if (relu_mask) {
      float yv[8];
      if (relu_mask == 2) {
        float sc[8], sh[8];
        ld8f(st + 2 * C + c, sc);
        ld8f(st + 3 * C + c, sh);
        bn_relu8(xv, sc, sh, yv);
      } else {
        unpack8(reinterpret_cast<const uint4*>(y)[i], yv);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = yv[e] > 0.f ? d[e] : 0.f;
    }
    ld8f(st + c, mean);
    ld8f(st + C + c, inv);
    ld8f(co + c, a);
    ld8f(co + C + c, b);
    ld8f(co + 2 * C + c, cc);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = a[e] * d[e] + b[e] + cc[e] * (xv[e] - mean[e]) * inv[e];
    reinterpret_cast<uint4*>(dx)[i] = pack8(d);
  }
}

// ---- inference (predict / evaluate through the native forward plan) ----------------------
// BatchNorm with the moving statistics: the same st rows bn_finalize writes from batch
// statistics (mean, 1/sqrt(var + eps), scale, shift), so every BN apply / fused residual /
// stem-pool kernel runs unchanged in inference mode.
__global__ __launch_bounds__(NT) void bn_infer_st_k(const float* __restrict__ rmean, const float* __restrict__ rvar,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    float eps, int C, float* __restrict__ st) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= C) return;
  const float m = rmean[c], inv = rsqrtf(rvar[c] + eps);
  const float sc = (gamma ? gamma[c] : 1.f) * inv;
  st[c] = m;
  st[C + c] = inv;
  st[2 * C + c] = sc;
  st[3 * C + c] = fmaf(-m, sc, beta ? beta[c] : 0.f);
}

// ---- launch heuristics ---------------------------------------------------------------------
// row-mapped apply kernels: about BN_UNR rows per thread (one batch of loads in flight)
int rows_grid(long M, int C, int cap = 16384) {
  const long rpi = NT / (C / 8);
  long g = (M + rpi * BN_UNR - 1) / (rpi * BN_UNR);
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
// grid cap of a row-mapped consumer that finalizes in its prologue (env DAMD_BN_FIN_GRID):
// every block pays the prologue, so fewer, longer-lived blocks.  ResNet-18 step: 2.707 ms
// uncapped (1568 blocks on layer 1), 2.671 at 512, 2.665 at 768.
int fin_rows_cap() {
  static int cap = [] {
    const char* e = getenv("DAMD_BN_FIN_GRID");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? v : 768;
  }();
  return cap;
}
// ... and at least DAMD_BN_FIN_MINKB KiB of each input tensor per block: every block reads
// all R x 4C accumulator words, which on the deep layers (C = 512: 128 KiB per block) was
// more than the block's share of the data
int fin_rows_grid(long M, int C) {
  static long minb = -1;
  if (minb < 0) {
    const char* e = getenv("DAMD_BN_FIN_MINKB");
    minb = e ? atol(e) * 1024 : 0;
  }
  int g = rows_grid(M, C, fin_rows_cap());
  if (minb > 0) {
    const long cap = ((long)M * C * 2 + minb - 1) / minb;
    if (g > cap) g = (int)(cap < 1 ? 1 : cap);
  }
  return g;
}

bool g_bn_reduce_reverse = false;

}  // namespace

hipError_t bn_finalize(const float* part, int T, int C, float count, const float* gamma, const float* beta, float eps,
                       float momentum, float* rmean, float* rvar, float* st, hipStream_t s) {
  if (C % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_finalize_k, dim3(C / 8), dim3(FT), 0, s, part, T, C, count, gamma, beta, eps,
                     momentum, rmean, rvar, st);
  return hipGetLastError();
}

hipError_t bn_apply(const uint16_t* x, const float* st, const uint16_t* r, const float* st2, int res_mode, int relu,
                    uint16_t* y, long M, int C, hipStream_t s, const BNFin* f1, const BNFin* f2) {
  const long n8 = M * C / 8;
  const BNFin a = f1 ? *f1 : kNoFin, b = (f2 && res_mode == 2) ? *f2 : kNoFin;
  if ((a.acc && !a.st) || (b.acc && !b.st) || ((a.acc || b.acc) && C > FIN_MAX_C)) return hipErrorInvalidValue;
  const size_t lds = (a.acc ? 4 * C * sizeof(float) : 0) + (b.acc ? 4 * C * sizeof(float) : 0);
  // (the f2 region starts at 4C: allocate it whenever f2 finalizes)
  const size_t lds2 = b.acc ? 8 * C * sizeof(float) : lds;
  if (NT % (C / 8) == 0) {
    hipLaunchKernelGGL(bn_apply_rows_k, dim3((a.acc || b.acc) ? fin_rows_grid(M, C) : rows_grid(M, C, 16384)), dim3(NT),
                       lds2, s, x, st, r, st2,
                       res_mode, relu, y, M, C, a, b);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(bn_apply_k, dim3(grid_for(n8, NT, (a.acc || b.acc) ? FIN_GRID_CAP : 8192)), dim3(NT), lds2, s,
                     x, st, r, st2, res_mode, relu, y, n8, C, a, b);
  return hipGetLastError();
}

int bn_bwd_blocks(long M, int C) {
  // target grid (DAMD_BN_BWD_BLOCKS, default 512): fewer blocks = fewer per-block partials
  // added into the fixed-point accumulators (4 atomics per channel and block).  ResNet-18
  // step, one box: 1024 blocks 2.736 ms, 512 2.718, 256 2.757
  static long target = 0;
  if (!target) {
    const char* e = getenv("DAMD_BN_BWD_BLOCKS");
    target = e ? atol(e) : 512;
    if (target < 64) target = 512;
  }
  const int rpi = NT / (C / 8);
  long rows = (M + target - 1) / target;
  if (rows < rpi) rows = rpi;
  // at least DAMD_BN_BWD_MINKB KiB of dy per block: on the small deep layers (M = 3136 rows
  // of 512 channels) the 512-block target gave 7 rows per block, and the 4C fixed-point
  // atomics of every block, not the 6 MB read, set the launch time
  static long minb = -1;
  if (minb < 0) {
    const char* e = getenv("DAMD_BN_BWD_MINKB");
    minb = e ? atol(e) * 1024 : 0;
  }
  const long row_bytes = (long)C * 2;
  if (minb > 0 && rows * row_bytes < minb) rows = (minb + row_bytes - 1) / row_bytes;
  return (int)((M + rows - 1) / rows);
}

void bn_reduce_reverse(bool on) { g_bn_reduce_reverse = on; }

hipError_t bn_bwd_reduce(const uint16_t* dy, const uint16_t* y, int relu_mask, const uint16_t* x, const float* st,
                         uint16_t* dz_out, float* part, int T, long M, int C, hipStream_t s, long long* acc,
                         int acc_reps) {
  if (C % 8 || C / 8 > NT || (!part && !acc) || acc_reps < 1) return hipErrorInvalidValue;
  const long rows = (M + T - 1) / T;
  if (relu_mask < 0 || relu_mask > 2) return hipErrorInvalidValue;
  auto k = relu_mask == 0 ? bn_bwd_reduce_k<0> : relu_mask == 1 ? bn_bwd_reduce_k<1> : bn_bwd_reduce_k<2>;
  hipLaunchKernelGGL(k, dim3(T), dim3(NT), 0, s, dy, y, x, st, dz_out, part, M, C, rows, acc, acc_reps,
                     g_bn_reduce_reverse ? 1 : 0);
  return hipGetLastError();
}

hipError_t bn_bwd_reduce_dual(const uint16_t* dy, const uint16_t* y, int relu_mask, const uint16_t* x,
                              const uint16_t* x2, const float* st, const float* st2, int T, long M, int C,
                              hipStream_t s, long long* acc, long long* acc2, int acc_reps) {
  if (C % 8 || C / 8 > NT || !acc || !acc2 || acc_reps < 1 || relu_mask < 0 || relu_mask > 1)
    return hipErrorInvalidValue;
  const long rows = (M + T - 1) / T;
  hipLaunchKernelGGL(bn_bwd_reduce2_k, dim3(T), dim3(NT), 0, s, dy, y, relu_mask, x, x2, st, st2, M, C, rows, acc,
                     acc2, acc_reps);
  return hipGetLastError();
}

hipError_t bn_bwd_apply_dual(const uint16_t* dy, const uint16_t* y, int relu_mask, const uint16_t* x,
                             const uint16_t* x2, const float* st, const float* st2, uint16_t* dx, uint16_t* dx2,
                             long M, int C, hipStream_t s, const BNBwdFin& bf, const BNBwdFin& bf2) {
  if (C % 8 || NT % (C / 8) || !bf.acc || !bf2.acc || !bf.co || !bf2.co || C > FIN_MAX_C || relu_mask < 0 ||
      relu_mask > 1)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_bwd_apply2_rows_k, dim3(fin_rows_grid(M, C)), dim3(NT), 6 * C * sizeof(float), s, dy, y,
                     relu_mask, x, x2, st, st2, dx, dx2, M, C, bf, bf2);
  return hipGetLastError();
}

hipError_t bn_bwd_finalize(const float* part, int T, int C, float count, const float* st, float* dgamma,
                           float* dbeta, float* co, hipStream_t s) {
  if (C % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_bwd_finalize_k, dim3(C / 8), dim3(FT), 0, s, part, T, C, count, st, dgamma, dbeta,
                     co);
  return hipGetLastError();
}

hipError_t bn_bwd_apply(const uint16_t* dy, const uint16_t* y, int relu_mask, const uint16_t* x, const float* st,
                        const float* co, uint16_t* dx, long M, int C, hipStream_t s, const BNBwdFin* bf) {
  const long n8 = M * C / 8;
  const BNBwdFin f = bf ? *bf : kNoBwdFin;
  if (f.acc && (!f.co || C > FIN_MAX_C)) return hipErrorInvalidValue;
  if (NT % (C / 8) == 0) {
    hipLaunchKernelGGL(bn_bwd_apply_rows_k, dim3(f.acc ? fin_rows_grid(M, C) : rows_grid(M, C, 16384)), dim3(NT),
                       f.acc ? 3 * C * sizeof(float) : 0, s, dy, y,
                       relu_mask, x, st, co, dx, M, C, f);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(bn_bwd_apply_k, dim3(grid_for(n8, NT, f.acc ? FIN_GRID_CAP : 8192)), dim3(NT),
                     f.acc ? 3 * C * sizeof(float) : 0, s, dy, y, relu_mask, x, st, co, dx, n8, C, f);
  return hipGetLastError();
}

hipError_t bn_infer_st(const float* rmean, const float* rvar, const float* gamma, const float* beta, float eps, int C,
                       float* st, hipStream_t s) {
  hipLaunchKernelGGL(bn_infer_st_k, dim3((C + NT - 1) / NT), dim3(NT), 0, s, rmean, rvar, gamma, beta, eps, C, st);
  return hipGetLastError();
}

}  // namespace damd
