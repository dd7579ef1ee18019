// Pooling of the generic path: max / average pooling (PoolGeo windows, TF 'same'
// semantics), global average pooling, and the stem fusion BatchNorm -> ReLU -> MaxPool with
// its backward (the BN-backward reduce / apply with the pool routing and the ReLU mask
// recomputed), pixel-centric for any geometry and quad-centric for the 3x3 / stride-2 pool.
// The stem kernels finalize the BatchNorm statistics in their prologue (layer_dev.h) when
// given fixed-point accumulators.  No atomics besides those accumulators: every output is
// written once.
#include "layer_dev.h"

namespace damd {
namespace {

__global__ __launch_bounds__(NT) void maxpool_fwd_k(const uint16_t* __restrict__ x, PoolGeo g,
                                                    uint16_t* __restrict__ y, uint8_t* __restrict__ arg) {
  const int cg = g.C / 8;
  const long total = (long)g.N * g.Ho * g.Wo * cg;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c8 = (int)(i % cg);
    long pix = i / cg;
    const int ow = (int)(pix % g.Wo);
    pix /= g.Wo;
    const int oh = (int)(pix % g.Ho);
    const int n = (int)(pix / g.Ho);
    float best[8];
    uint8_t bi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { best[e] = -INFINITY; bi[e] = 0; }
    for (int kh = 0; kh < g.ph; ++kh) {
      const int ih = oh * g.sh - g.pt + kh;
      if ((unsigned)ih >= (unsigned)g.H) continue;
      for (int kw = 0; kw < g.pw; ++kw) {
        const int iw = ow * g.sw - g.pl + kw;
        if ((unsigned)iw >= (unsigned)g.W) continue;
        float v[8];
        unpack8(reinterpret_cast<const uint4*>(x)[(((long)n * g.H + ih) * g.W + iw) * cg + c8], v);
        const uint8_t idx = (uint8_t)(kh * g.pw + kw);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (v[e] > best[e]) { best[e] = v[e]; bi[e] = idx; }
      }
    }
    reinterpret_cast<uint4*>(y)[i] = pack8(best);
    uint2 a;
    a.x = bi[0] | (bi[1] << 8) | (bi[2] << 16) | ((uint32_t)bi[3] << 24);
    a.y = bi[4] | (bi[5] << 8) | (bi[6] << 16) | ((uint32_t)bi[7] << 24);
    reinterpret_cast<uint2*>(arg)[i] = a;
  }
}

__global__ __launch_bounds__(NT) void maxpool_bwd_k(const uint16_t* __restrict__ dy, const uint8_t* __restrict__ arg,
                                                    PoolGeo g, uint16_t* __restrict__ dx) {
  const int cg = g.C / 8;
  const long total = (long)g.N * g.H * g.W * cg;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c8 = (int)(i % cg);
    long pix = i / cg;
    const int iw = (int)(pix % g.W);
    pix /= g.W;
    const int ih = (int)(pix % g.H);
    const int n = (int)(pix / g.H);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    // output rows whose window covers ih: oh*sh - pt <= ih <= oh*sh - pt + ph - 1
    const int ohlo = max(0, (ih + g.pt - g.ph + g.sh) / g.sh), ohhi = min(g.Ho - 1, (ih + g.pt) / g.sh);
    const int owlo = max(0, (iw + g.pl - g.pw + g.sw) / g.sw), owhi = min(g.Wo - 1, (iw + g.pl) / g.sw);
    for (int oh = ohlo; oh <= ohhi; ++oh) {
      const int kh = ih - (oh * g.sh - g.pt);
      if (kh < 0 || kh >= g.ph) continue;
      for (int ow = owlo; ow <= owhi; ++ow) {
        const int kw = iw - (ow * g.sw - g.pl);
        if (kw < 0 || kw >= g.pw) continue;
        const long o = (((long)n * g.Ho + oh) * g.Wo + ow) * cg + c8;
        const uint2 a = reinterpret_cast<const uint2*>(arg)[o];
        const uint8_t me = (uint8_t)(kh * g.pw + kw);
        float d[8];
        unpack8(reinterpret_cast<const uint4*>(dy)[o], d);
        const uint32_t w[2] = {a.x, a.y};
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (((w[e >> 2] >> (8 * (e & 3))) & 0xff) == me) acc[e] += d[e];
      }
    }
    reinterpret_cast<uint4*>(dx)[i] = pack8(acc);
  }
}

// Average pooling (Keras AveragePooling2D): the divisor is the number of in-bounds taps, so
// 'same' windows that overhang the border average only real pixels (TF's avg_pool) and
// 'valid' windows divide by ph*pw.  The backward is a gather over the output windows that
// cover each input pixel (no atomics, every dx written once).
__device__ __forceinline__ float pool_inv_count(int oh, int ow, const PoolGeo& g) {
  const int h0 = oh * g.sh - g.pt, w0 = ow * g.sw - g.pl;
  const int nh = min(h0 + g.ph, g.H) - max(h0, 0), nw = min(w0 + g.pw, g.W) - max(w0, 0);
  return 1.f / (float)(nh * nw);
}

__global__ __launch_bounds__(NT) void avgpool_fwd_k(const uint16_t* __restrict__ x, PoolGeo g,
                                                    uint16_t* __restrict__ y) {
  const int cg = g.C / 8;
  const long total = (long)g.N * g.Ho * g.Wo * cg;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c8 = (int)(i % cg);
    long pix = i / cg;
    const int ow = (int)(pix % g.Wo);
    pix /= g.Wo;
    const int oh = (int)(pix % g.Ho);
    const int n = (int)(pix / g.Ho);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int kh = 0; kh < g.ph; ++kh) {
      const int ih = oh * g.sh - g.pt + kh;
      if ((unsigned)ih >= (unsigned)g.H) continue;
      for (int kw = 0; kw < g.pw; ++kw) {
        const int iw = ow * g.sw - g.pl + kw;
        if ((unsigned)iw >= (unsigned)g.W) continue;
        float v[8];
        unpack8(reinterpret_cast<const uint4*>(x)[(((long)n * g.H + ih) * g.W + iw) * cg + c8], v);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += v[e];
      }
    }
    const float inv = pool_inv_count(oh, ow, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= inv;
    reinterpret_cast<uint4*>(y)[i] = pack8(acc);
  }
}

__global__ __launch_bounds__(NT) void avgpool_bwd_k(const uint16_t* __restrict__ dy, PoolGeo g,
                                                    uint16_t* __restrict__ dx) {
  const int cg = g.C / 8;
  const long total = (long)g.N * g.H * g.W * cg;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c8 = (int)(i % cg);
    long pix = i / cg;
    const int iw = (int)(pix % g.W);
    pix /= g.W;
    const int ih = (int)(pix % g.H);
    const int n = (int)(pix / g.H);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    const int ohlo = max(0, (ih + g.pt - g.ph + g.sh) / g.sh), ohhi = min(g.Ho - 1, (ih + g.pt) / g.sh);
    const int owlo = max(0, (iw + g.pl - g.pw + g.sw) / g.sw), owhi = min(g.Wo - 1, (iw + g.pl) / g.sw);
    for (int oh = ohlo; oh <= ohhi; ++oh) {
      const int kh = ih - (oh * g.sh - g.pt);
      if (kh < 0 || kh >= g.ph) continue;
      for (int ow = owlo; ow <= owhi; ++ow) {
        const int kw = iw - (ow * g.sw - g.pl);
        if (kw < 0 || kw >= g.pw) continue;
        float d[8];
        unpack8(reinterpret_cast<const uint4*>(dy)[(((long)n * g.Ho + oh) * g.Wo + ow) * cg + c8], d);
        const float inv = pool_inv_count(oh, ow, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += d[e] * inv;
      }
    }
    reinterpret_cast<uint4*>(dx)[i] = pack8(acc);
  }
}

// ---- stem fusion: BatchNorm -> ReLU -> MaxPool without the normalised tensor ----------
// Forward: the pool reads the conv output x and normalises on the fly (the BN+ReLU output
// is never stored); each candidate is rounded to bf16 exactly as bn_apply stores it, so
// max / argmax equal the unfused pair's.  Backward: the pool's gradient routing and the
// ReLU mask are recomputed from (dy_pool, argmax, x, BN scale/shift) in both BN-backward
// passes, so neither the 4x larger un-pooled gradient nor the ReLU output is stored.

__global__ __launch_bounds__(NT) void bn_relu_maxpool_fwd_k(const uint16_t* __restrict__ x,
                                                            const float* st_in, PoolGeo g,
                                                            uint16_t* __restrict__ y, uint8_t* __restrict__ arg,
                                                            BNFin f) {
  extern __shared__ float sfin[];
  const float* st = bn_fin_prologue(f, g.C, sfin, st_in);
  const int cg = g.C / 8;
  const long total = (long)g.N * g.Ho * g.Wo * cg;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c8 = (int)(i % cg);
    long pix = i / cg;
    const int ow = (int)(pix % g.Wo);
    pix /= g.Wo;
    const int oh = (int)(pix % g.Ho);
    const int n = (int)(pix / g.Ho);
    float sc[8], sh[8];
    ld8f(st + 2 * g.C + c8 * 8, sc);
    ld8f(st + 3 * g.C + c8 * 8, sh);
    float best[8];
    uint8_t bi[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { best[e] = -INFINITY; bi[e] = 0; }
    for (int kh = 0; kh < g.ph; ++kh) {
      const int ih = oh * g.sh - g.pt + kh;
      if ((unsigned)ih >= (unsigned)g.H) continue;
      for (int kw = 0; kw < g.pw; ++kw) {
        const int iw = ow * g.sw - g.pl + kw;
        if ((unsigned)iw >= (unsigned)g.W) continue;
        float xv[8], v[8];
        unpack8(reinterpret_cast<const uint4*>(x)[(((long)n * g.H + ih) * g.W + iw) * cg + c8], xv);
        bn_relu8(xv, sc, sh, v);
        const uint8_t idx = (uint8_t)(kh * g.pw + kw);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (v[e] > best[e]) { best[e] = v[e]; bi[e] = idx; }
      }
    }
    reinterpret_cast<uint4*>(y)[i] = pack8(best);
    uint2 a;
    a.x = bi[0] | (bi[1] << 8) | (bi[2] << 16) | ((uint32_t)bi[3] << 24);
    a.y = bi[4] | (bi[5] << 8) | (bi[6] << 16) | ((uint32_t)bi[7] << 24);
    reinterpret_cast<uint2*>(arg)[i] = a;
  }
}

// 3x3/s2 pool, H = 2 Ho, W = 2 Wo, Ho and Wo even: one thread per 2x2 block of outputs.
// Its 5x5 input patch is walked row by row (5 loads + BN/ReLU each), and every row updates
// the outputs whose windows contain it, taps in ascending (kh, kw) order with the same
// strict '>' as bn_relu_maxpool_fwd_k, so values and argmax codes are bitwise equal; 25
// loads and normalisations per 4 outputs instead of 36.
template <int PT, int PL>
__global__ __launch_bounds__(NT) void bn_relu_maxpool_fwd_q_k(const uint16_t* __restrict__ x,
                                                              const float* st_in, PoolGeo g,
                                                              uint16_t* __restrict__ y, uint8_t* __restrict__ arg,
                                                              BNFin f) {
  extern __shared__ float sfin[];
  const float* st = bn_fin_prologue(f, g.C, sfin, st_in);
  const int cg = g.C / 8;
  const int Ho2 = g.Ho / 2, Wo2 = g.Wo / 2;
  const long total = (long)g.N * Ho2 * Wo2 * cg;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c8 = (int)(i % cg);
    long q = i / cg;
    const int b2 = (int)(q % Wo2);
    q /= Wo2;
    const int a2 = (int)(q % Ho2);
    const int n = (int)(q / Ho2);
    float sc[8], sh[8];
    ld8f(st + 2 * g.C + c8 * 8, sc);
    ld8f(st + 3 * g.C + c8 * 8, sh);
    float best[4][8];
    uint32_t code[4][2];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
#pragma unroll
      for (int e = 0; e < 8; ++e) best[o][e] = -INFINITY;
      code[o][0] = code[o][1] = 0u;
    }
    const int ih0 = 4 * a2 - PT, iw0 = 4 * b2 - PL;
#pragma unroll
    for (int pr = 0; pr < 5; ++pr) {
      const int ih = ih0 + pr;
      if ((unsigned)ih >= (unsigned)g.H) continue;
      float v[5][8];
      bool ok[5];
#pragma unroll
      for (int pc = 0; pc < 5; ++pc) {
        const int iw = iw0 + pc;
        ok[pc] = (unsigned)iw < (unsigned)g.W;
        float xv[8];
        unpack8(reinterpret_cast<const uint4*>(x)[(((long)n * g.H + ih) * g.W + (ok[pc] ? iw : 0)) * cg + c8], xv);
        bn_relu8(xv, sc, sh, v[pc]);
      }
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int kh = pr - 2 * r;
        if (kh < 0 || kh > 2) continue;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int o = 2 * r + c;
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const int pc = 2 * c + kw;
            if (!ok[pc]) continue;
            const uint32_t idx = (uint32_t)(kh * 3 + kw);
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (v[pc][e] > best[o][e]) {
                best[o][e] = v[pc][e];
                code[o][e >> 2] = (code[o][e >> 2] & ~(0xffu << (8 * (e & 3)))) | (idx << (8 * (e & 3)));
              }
          }
        }
      }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const long oi = (((long)n * g.Ho + 2 * a2 + (o >> 1)) * g.Wo + 2 * b2 + (o & 1)) * cg + c8;
      reinterpret_cast<uint4*>(y)[oi] = pack8(best[o]);
      reinterpret_cast<uint2*>(arg)[oi] = uint2{code[o][0], code[o][1]};
    }
  }
}

// gradient reaching input pixel (n, ih, iw), channels 8*c8.. through the max-pool windows
// (fp32 sum, then rounded to bf16 as maxpool_bwd stores it)
__device__ __forceinline__ void pool_grad8(const uint16_t* __restrict__ dy, const uint8_t* __restrict__ arg,
                                           const PoolGeo& g, int n, int ih, int iw, int c8, float* acc) {
  const int cg = g.C / 8;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  const int ohlo = max(0, (ih + g.pt - g.ph + g.sh) / g.sh), ohhi = min(g.Ho - 1, (ih + g.pt) / g.sh);
  const int owlo = max(0, (iw + g.pl - g.pw + g.sw) / g.sw), owhi = min(g.Wo - 1, (iw + g.pl) / g.sw);
  for (int oh = ohlo; oh <= ohhi; ++oh) {
    const int kh = ih - (oh * g.sh - g.pt);
    if (kh < 0 || kh >= g.ph) continue;
    for (int ow = owlo; ow <= owhi; ++ow) {
      const int kw = iw - (ow * g.sw - g.pl);
      if (kw < 0 || kw >= g.pw) continue;
      const long o = (((long)n * g.Ho + oh) * g.Wo + ow) * cg + c8;
      const uint2 a = reinterpret_cast<const uint2*>(arg)[o];
      const uint8_t me = (uint8_t)(kh * g.pw + kw);
      float d[8];
      unpack8(reinterpret_cast<const uint4*>(dy)[o], d);
      const uint32_t w[2] = {a.x, a.y};
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (((w[e >> 2] >> (8 * (e & 3))) & 0xff) == me) acc[e] += d[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = bf2f(f2bf(acc[e]));
}

// masked upstream gradient of the BN output at input row `row` (flattened n, ih, iw)
__device__ __forceinline__ void stem_dy8(const uint16_t* __restrict__ dpool, const uint8_t* __restrict__ arg,
                                         const PoolGeo& g, long row, int c8, const float* xv, const float* sc,
                                         const float* sh, float* d) {
  const int iw = (int)(row % g.W);
  const long t = row / g.W;
  const int ih = (int)(t % g.H), n = (int)(t / g.H);
  pool_grad8(dpool, arg, g, n, ih, iw, c8, d);
  float yv[8];
  bn_relu8(xv, sc, sh, yv);
#pragma unroll
  for (int e = 0; e < 8; ++e) d[e] = yv[e] > 0.f ? d[e] : 0.f;
}

__global__ __launch_bounds__(NT) void pool_bn_bwd_reduce_k(const uint16_t* __restrict__ dpool,
                                                           const uint8_t* __restrict__ arg, PoolGeo g,
                                                           const uint16_t* __restrict__ x, const float* __restrict__ st,
                                                           float* __restrict__ part, long M, long rows_per_block,
                                                           long long* __restrict__ acc, int reps) {
  __shared__ float red[2][NT * 8];
  const int C = g.C, cg = C / 8, t = threadIdx.x;
  const int rpi = NT / cg;
  const int gq = t % cg, rr = t / cg;
  const int c = gq * 8;
  float s0[8], s1[8], mean[8], inv[8], sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s0[e] = s1[e] = 0.f;
  ld8f(st + c, mean);
  ld8f(st + C + c, inv);
  ld8f(st + 2 * C + c, sc);
  ld8f(st + 3 * C + c, sh);
  const long r0 = blockIdx.x * rows_per_block, r1 = min(M, r0 + rows_per_block);
  if (rr < rpi) {
    for (long row = r0 + rr; row < r1; row += rpi) {
      float xv[8], d[8];
      unpack8(reinterpret_cast<const uint4*>(x)[(row * C + c) / 8], xv);
      stem_dy8(dpool, arg, g, row, gq, xv, sc, sh, d);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s0[e] += d[e];
        s1[e] += d[e] * (xv[e] - mean[e]) * inv[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[0][t * 8 + e] = rr < rpi ? s0[e] : 0.f;
    red[1][t * 8 + e] = rr < rpi ? s1[e] : 0.f;
  }
  __syncthreads();
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

__global__ __launch_bounds__(NT) void pool_bn_bwd_apply_k(const uint16_t* __restrict__ dpool,
                                                          const uint8_t* __restrict__ arg, PoolGeo g,
                                                          const uint16_t* __restrict__ x, const float* __restrict__ st,
                                                          const float* co_in, uint16_t* __restrict__ dx,
                                                          long n8, BNBwdFin bf) {
  extern __shared__ float sfin[];
  const float* co = bn_bwd_fin_prologue(bf, g.C, st, sfin, co_in);
  const int C = g.C, cg = C / 8;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += (long)gridDim.x * NT) {
    const int c8 = (int)(i % cg), c = c8 * 8;
    const long row = i / cg;
    float xv[8], d[8], mean[8], inv[8], sc[8], sh[8], a[8], b[8], cc[8];
    unpack8(reinterpret_cast<const uint4*>(x)[i], xv);
    ld8f(st + c, mean);
    ld8f(st + C + c, inv);
    ld8f(st + 2 * C + c, sc);
    ld8f(st + 3 * C + c, sh);
    stem_dy8(dpool, arg, g, row, c8, xv, sc, sh, d);
    ld8f(co + c, a);
    ld8f(co + C + c, b);
    ld8f(co + 2 * C + c, cc);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = a[e] * d[e] + b[e] + cc[e] * (xv[e] - mean[e]) * inv[e];
    reinterpret_cast<uint4*>(dx)[i] = pack8(d);
  }
}

// ---- stem backward, 3x3/s2 pool with H = 2 Ho, W = 2 Wo: one thread per 2x2 input quad --
// Pixel-centric gathers (above) load every covering pool window per input pixel: 2.25
// windows x (16 B gradient + 8 B argmax code) per pixel on average, each a dependent
// chain.  The 2x2 quad (2a..2a+1, 2b..2b+1) is covered by exactly the windows
// {a-1+PT, a+PT} x {b-1+PL, b+PL}: one thread loads those 4 windows once (8 independent
// loads) and routes them to its 4 pixels.  Window (wr, wc) reaches pixel (py, px) at tap
// kh = py + 2 - PT - 2 wr, kw = px + 2 - PL - 2 wc (valid when in [0, 2]); taps are
// accumulated in ascending (oh, ow) order exactly as pool_grad8 does, so the routed
// gradient and dx are bitwise those of the pixel-centric kernels for the same BN
// coefficients.
struct Quad8 {
  float d[4][8];  // routed (bf16-rounded) pool gradient of pixels (py, px) = (q >> 1, q & 1)
};

template <int PT, int PL>
__device__ __forceinline__ void quad_route8(const uint16_t* __restrict__ dpool, const uint8_t* __restrict__ arg,
                                            const PoolGeo& g, int n, int a, int b, int c8, Quad8& o) {
  const int cg = g.C / 8;
  float dw[2][2][8];
  uint32_t aw[2][2][2];
  // the four windows are loaded unconditionally at clamped coordinates and the out-of-range
  // ones neutralised after (a load under the edge branch cost its own round trip: the
  // ResNet-18 stem's backward apply 66 -> 59 us)
  uint4 dq[2][2];
  uint2 aq[2][2];
#pragma unroll
  for (int wr = 0; wr < 2; ++wr) {
#pragma unroll
    for (int wc = 0; wc < 2; ++wc) {
      const int oh = min(max(a - 1 + PT + wr, 0), g.Ho - 1), ow = min(max(b - 1 + PL + wc, 0), g.Wo - 1);
      const long w = (((long)n * g.Ho + oh) * g.Wo + ow) * cg + c8;
      dq[wr][wc] = reinterpret_cast<const uint4*>(dpool)[w];
      aq[wr][wc] = reinterpret_cast<const uint2*>(arg)[w];
    }
  }
#pragma unroll
  for (int wr = 0; wr < 2; ++wr) {
#pragma unroll
    for (int wc = 0; wc < 2; ++wc) {
      const int oh = a - 1 + PT + wr, ow = b - 1 + PL + wc;
      const bool ok = (unsigned)oh < (unsigned)g.Ho && (unsigned)ow < (unsigned)g.Wo;
      unpack8(dq[wr][wc], dw[wr][wc]);
      aw[wr][wc][0] = ok ? aq[wr][wc].x : 0xffffffffu;  // code 255 never matches a tap
      aw[wr][wc][1] = ok ? aq[wr][wc].y : 0xffffffffu;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int py = q >> 1, px = q & 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.d[q][e] = 0.f;
#pragma unroll
    for (int wr = 0; wr < 2; ++wr) {
      const int kh = py + 2 - PT - 2 * wr;
      if (kh < 0 || kh > 2) continue;
#pragma unroll
      for (int wc = 0; wc < 2; ++wc) {
        const int kw = px + 2 - PL - 2 * wc;
        if (kw < 0 || kw > 2) continue;
        const uint32_t me = (uint32_t)(kh * 3 + kw);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (((aw[wr][wc][e >> 2] >> (8 * (e & 3))) & 0xffu) == me) o.d[q][e] += dw[wr][wc][e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) o.d[q][e] = bf2f(f2bf(o.d[q][e]));
  }
}

template <int PT, int PL>
__global__ __launch_bounds__(NT) void pool_bn_bwd_reduce_q_k(const uint16_t* __restrict__ dpool,
                                                             const uint8_t* __restrict__ arg, PoolGeo g,
                                                             const uint16_t* __restrict__ x,
                                                             const float* __restrict__ st, float* __restrict__ part,
                                                             long nquad, long quads_per_block, long long* __restrict__ acc,
                                                             int reps) {
  __shared__ float red[2][NT * 8];
  const int C = g.C, cg = C / 8, t = threadIdx.x;
  const int rpi = NT / cg;
  const int gq = t % cg, rr = t / cg;
  const int c = gq * 8;
  float s0[8], s1[8], mean[8], inv[8], sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s0[e] = s1[e] = 0.f;
  ld8f(st + c, mean);
  ld8f(st + C + c, inv);
  ld8f(st + 2 * C + c, sc);
  ld8f(st + 3 * C + c, sh);
  const long q0 = blockIdx.x * quads_per_block, q1 = min(nquad, q0 + quads_per_block);
  if (rr < rpi) {
    for (long qd = q0 + rr; qd < q1; qd += rpi) {
      const int b = (int)(qd % g.Wo);
      const long tq = qd / g.Wo;
      const int a = (int)(tq % g.Ho), n = (int)(tq / g.Ho);
      float xv[4][8];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long pix = ((long)n * g.H + 2 * a + (q >> 1)) * g.W + 2 * b + (q & 1);
        unpack8(reinterpret_cast<const uint4*>(x)[pix * cg + gq], xv[q]);
      }
      Quad8 r;
      quad_route8<PT, PL>(dpool, arg, g, n, a, b, gq, r);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float yv[8];
        bn_relu8(xv[q], sc, sh, yv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = yv[e] > 0.f ? r.d[q][e] : 0.f;
          s0[e] += d;
          s1[e] += d * (xv[q][e] - mean[e]) * inv[e];
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
  for (int ch = t; ch < C; ch += NT) {
    const int gg = ch / 8, e = ch % 8;
    float sa = 0.f, sb = 0.f;
    for (int q = 0; q < rpi; ++q) {
      sa += red[0][(q * cg + gg) * 8 + e];
      sb += red[1][(q * cg + gg) * 8 + e];
    }
    put_partial(part, acc, reps, C, ch, sa, sb);
  }
}

template <int PT, int PL>
__global__ __launch_bounds__(NT) void pool_bn_bwd_apply_q_k(const uint16_t* __restrict__ dpool,
                                                            const uint8_t* __restrict__ arg, PoolGeo g,
                                                            const uint16_t* __restrict__ x,
                                                            const float* __restrict__ st,
                                                            const float* co_in, uint16_t* __restrict__ dx,
                                                            long nq8, BNBwdFin bf) {
  extern __shared__ float sfin[];
  const float* co = bn_bwd_fin_prologue(bf, g.C, st, sfin, co_in);
  const int C = g.C, cg = C / 8;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < nq8; i += (long)gridDim.x * NT) {
    const int c8 = (int)(i % cg), c = c8 * 8;
    const long qd = i / cg;
    const int b = (int)(qd % g.Wo);
    const long tq = qd / g.Wo;
    const int a = (int)(tq % g.Ho), n = (int)(tq / g.Ho);
    long pix[4];
    float xv[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pix[q] = ((long)n * g.H + 2 * a + (q >> 1)) * g.W + 2 * b + (q & 1);
      unpack8(reinterpret_cast<const uint4*>(x)[pix[q] * cg + c8], xv[q]);
    }
    Quad8 r;
    quad_route8<PT, PL>(dpool, arg, g, n, a, b, c8, r);
    float mean[8], inv[8], sc[8], sh[8], ca[8], cb[8], cc[8];
    ld8f(st + c, mean);
    ld8f(st + C + c, inv);
    ld8f(st + 2 * C + c, sc);
    ld8f(st + 3 * C + c, sh);
    ld8f(co + c, ca);
    ld8f(co + C + c, cb);
    ld8f(co + 2 * C + c, cc);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float yv[8], d[8];
      bn_relu8(xv[q], sc, sh, yv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float dm = yv[e] > 0.f ? r.d[q][e] : 0.f;
        d[e] = ca[e] * dm + cb[e] + cc[e] * (xv[q][e] - mean[e]) * inv[e];
      }
      reinterpret_cast<uint4*>(dx)[pix[q] * cg + c8] = pack8(d);
    }
  }
}

__host__ __forceinline__ bool quad_pool_geo(const PoolGeo& g) {
  return g.ph == 3 && g.pw == 3 && g.sh == 2 && g.sw == 2 && (g.pt == 0 || g.pt == 1) && (g.pl == 0 || g.pl == 1) &&
         g.H == 2 * g.Ho && g.W == 2 * g.Wo;
}

__global__ __launch_bounds__(NT) void gap_fwd_k(const uint16_t* __restrict__ x, int N, int HW, int C, void* y,
                                                int y_f32) {
  const int cg = C / 8;
  const long total = (long)N * cg;
  const float inv = 1.f / HW;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c8 = (int)(i % cg), n = (int)(i / cg);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int p = 0; p < HW; ++p) {
      float v[8];
      unpack8(reinterpret_cast<const uint4*>(x)[((long)n * HW + p) * cg + c8], v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] *= inv;
    if (y_f32) {
      float* o = (float*)y + (long)n * C + c8 * 8;
      *reinterpret_cast<float4*>(o) = float4{acc[0], acc[1], acc[2], acc[3]};
      *reinterpret_cast<float4*>(o + 4) = float4{acc[4], acc[5], acc[6], acc[7]};
    } else {
      reinterpret_cast<uint4*>(y)[i] = pack8(acc);
    }
  }
}

// One image per block, the pixels split over G = NT / cg thread groups (ResNet-18's 7x7x512
// head: 4 groups of ~12 pixels, 64 blocks) instead of one thread walking all HW pixels per
// channel group (16 blocks, a 49-long load chain each); partials combined in group order.
__global__ __launch_bounds__(NT) void gap_fwd_img_k(const uint16_t* __restrict__ x, int HW, int C, void* y,
                                                    int y_f32) {
  __shared__ float part[NT * 8];
  const int cg = C / 8, G = NT / cg, t = threadIdx.x, n = blockIdx.x;
  const int c8 = t % cg, g = t / cg;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (g < G) {
    for (int p = g; p < HW; p += G) {
      float v[8];
      unpack8(reinterpret_cast<const uint4*>(x)[((long)n * HW + p) * cg + c8], v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[t * 8 + e] = acc[e];
  __syncthreads();
  if (t >= cg) return;
  float r[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = 0.f;
  for (int q = 0; q < G; ++q)
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] += part[(q * cg + t) * 8 + e];
  const float inv = 1.f / HW;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] *= inv;
  if (y_f32) {
    float* o = (float*)y + (long)n * C + t * 8;
    *reinterpret_cast<float4*>(o) = float4{r[0], r[1], r[2], r[3]};
    *reinterpret_cast<float4*>(o + 4) = float4{r[4], r[5], r[6], r[7]};
  } else {
    reinterpret_cast<uint4*>(y)[(long)n * cg + t] = pack8(r);
  }
}

__global__ __launch_bounds__(NT) void gap_bwd_k(const void* dy, int dy_f32, int N, int HW, int C,
                                                uint16_t* __restrict__ dx) {
  const int cg = C / 8;
  const long total = (long)N * HW * cg;
  const float inv = 1.f / HW;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c8 = (int)(i % cg);
    const int n = (int)(i / ((long)cg * HW));
    float d[8];
    if (dy_f32) ld8f((const float*)dy + (long)n * C + c8 * 8, d);
    else unpack8(reinterpret_cast<const uint4*>(dy)[(long)n * cg + c8], d);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] *= inv;
    reinterpret_cast<uint4*>(dx)[i] = pack8(d);
  }
}

}  // namespace

hipError_t maxpool_fwd(const uint16_t* x, const PoolGeo& g, uint16_t* y, uint8_t* arg, hipStream_t s) {
  if (g.C % 8 || g.ph * g.pw > 255) return hipErrorInvalidValue;
  hipLaunchKernelGGL(maxpool_fwd_k, dim3(grid_for((long)g.N * g.Ho * g.Wo * g.C / 8)), dim3(NT), 0, s, x, g, y, arg);
  return hipGetLastError();
}

hipError_t maxpool_bwd(const uint16_t* dy, const uint8_t* arg, const PoolGeo& g, uint16_t* dx, hipStream_t s) {
  if (g.C % 8 || g.ph * g.pw > 255) return hipErrorInvalidValue;  // (tap codes are uint8, as the forward's)
  hipLaunchKernelGGL(maxpool_bwd_k, dim3(grid_for((long)g.N * g.H * g.W * g.C / 8)), dim3(NT), 0, s, dy, arg, g, dx);
  return hipGetLastError();
}

hipError_t avgpool_fwd(const uint16_t* x, const PoolGeo& g, uint16_t* y, hipStream_t s) {
  if (g.C % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(avgpool_fwd_k, dim3(grid_for((long)g.N * g.Ho * g.Wo * g.C / 8)), dim3(NT), 0, s, x, g, y);
  return hipGetLastError();
}

hipError_t avgpool_bwd(const uint16_t* dy, const PoolGeo& g, uint16_t* dx, hipStream_t s) {
  if (g.C % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(avgpool_bwd_k, dim3(grid_for((long)g.N * g.H * g.W * g.C / 8)), dim3(NT), 0, s, dy, g, dx);
  return hipGetLastError();
}

hipError_t bn_relu_maxpool_fwd(const uint16_t* x, const float* st, const PoolGeo& g, uint16_t* y, uint8_t* arg,
                               hipStream_t s, const BNFin* fp) {
  if (g.C % 8 || g.ph * g.pw > 255) return hipErrorInvalidValue;
  const BNFin f = fp ? *fp : kNoFin;
  if (f.acc && (!f.st || g.C > FIN_MAX_C)) return hipErrorInvalidValue;
  const int cap = f.acc ? FIN_GRID_CAP : 8192;
  const size_t lds = f.acc ? 4 * g.C * sizeof(float) : 0;
  if (quad_pool_geo(g) && g.Ho % 2 == 0 && g.Wo % 2 == 0) {
    auto k = g.pt ? (g.pl ? bn_relu_maxpool_fwd_q_k<1, 1> : bn_relu_maxpool_fwd_q_k<1, 0>)
                  : (g.pl ? bn_relu_maxpool_fwd_q_k<0, 1> : bn_relu_maxpool_fwd_q_k<0, 0>);
    hipLaunchKernelGGL(k, dim3(grid_for((long)g.N * g.Ho * g.Wo * g.C / 32, NT, cap)), dim3(NT), lds, s, x, st, g, y,
                       arg, f);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(bn_relu_maxpool_fwd_k, dim3(grid_for((long)g.N * g.Ho * g.Wo * g.C / 8, NT, cap)), dim3(NT), lds,
                     s, x, st, g, y, arg, f);
  return hipGetLastError();
}

hipError_t pool_bn_bwd_reduce(const uint16_t* dpool, const uint8_t* arg, const PoolGeo& g, const uint16_t* x,
                              const float* st, float* part, int T, hipStream_t s, long long* acc, int acc_reps) {
  const int C = g.C;
  if (C % 8 || C / 8 > NT || g.ph * g.pw > 255 || (!part && !acc) || acc_reps < 1) return hipErrorInvalidValue;
  const long M = (long)g.N * g.H * g.W, rows = (M + T - 1) / T;
  if (quad_pool_geo(g)) {
    const long nq = (long)g.N * g.Ho * g.Wo, qpb = (nq + T - 1) / T;
    auto k = g.pt ? (g.pl ? pool_bn_bwd_reduce_q_k<1, 1> : pool_bn_bwd_reduce_q_k<1, 0>)
                  : (g.pl ? pool_bn_bwd_reduce_q_k<0, 1> : pool_bn_bwd_reduce_q_k<0, 0>);
    hipLaunchKernelGGL(k, dim3(T), dim3(NT), 0, s, dpool, arg, g, x, st, part, nq, qpb, acc, acc_reps);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(pool_bn_bwd_reduce_k, dim3(T), dim3(NT), 0, s, dpool, arg, g, x, st, part, M, rows, acc,
                     acc_reps);
  return hipGetLastError();
}

hipError_t pool_bn_bwd_apply(const uint16_t* dpool, const uint8_t* arg, const PoolGeo& g, const uint16_t* x,
                             const float* st, const float* co, uint16_t* dx, hipStream_t s, const BNBwdFin* bfp) {
  const int C = g.C;
  if (C % 8 || g.ph * g.pw > 255) return hipErrorInvalidValue;
  const BNBwdFin f = bfp ? *bfp : kNoBwdFin;
  if (f.acc && (!f.co || C > FIN_MAX_C)) return hipErrorInvalidValue;
  const int cap = f.acc ? FIN_GRID_CAP : 8192;
  const size_t lds = f.acc ? 3 * C * sizeof(float) : 0;
  const long n8 = (long)g.N * g.H * g.W * C / 8;
  if (quad_pool_geo(g)) {
    const long nq8 = (long)g.N * g.Ho * g.Wo * C / 8;
    auto k = g.pt ? (g.pl ? pool_bn_bwd_apply_q_k<1, 1> : pool_bn_bwd_apply_q_k<1, 0>)
                  : (g.pl ? pool_bn_bwd_apply_q_k<0, 1> : pool_bn_bwd_apply_q_k<0, 0>);
    hipLaunchKernelGGL(k, dim3(grid_for(nq8, NT, cap)), dim3(NT), lds, s, dpool, arg, g, x, st, co, dx, nq8, f);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(pool_bn_bwd_apply_k, dim3(grid_for(n8, NT, cap)), dim3(NT), lds, s, dpool, arg, g, x, st, co, dx,
                     n8, f);
  return hipGetLastError();
}

hipError_t gap_fwd(const uint16_t* x, int N, int HW, int C, void* y, int y_f32, hipStream_t s) {
  if (C % 8) return hipErrorInvalidValue;
  if (C / 8 <= NT / 2 && HW >= 8) {
    hipLaunchKernelGGL(gap_fwd_img_k, dim3(N), dim3(NT), 0, s, x, HW, C, y, y_f32);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(gap_fwd_k, dim3(grid_for((long)N * C / 8)), dim3(NT), 0, s, x, N, HW, C, y, y_f32);
  return hipGetLastError();
}

hipError_t gap_bwd(const void* dy, int dy_f32, int N, int HW, int C, uint16_t* dx, hipStream_t s) {
  if (C % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gap_bwd_k, dim3(grid_for((long)N * HW * C / 8)), dim3(NT), 0, s, dy, dy_f32, N, HW, C, dx);
  return hipGetLastError();
}

}  // namespace damd
