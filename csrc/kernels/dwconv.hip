// Depthwise convolution of the generic path (DepthwiseConv2D and the depthwise half of
// SeparableConv2D, depth_multiplier 1): forward, backprop-input and weight gradient over
// PoolGeo windows (ph x pw the kernel, TF 'same' semantics: the extra padding row / column
// below / right).  x [N][H][W][C] bf16, taps w [ph*pw][C] bf16, y [N][Ho][Wo][C] bf16; one
// thread moves one 16-byte vector of 8 channels.  Memory-bound: every activation vector is
// read from memory once per launch (the taps that overlap hit in L1 / L2), the taps
// themselves are [ph*pw][C] bf16 and stay cached.  No atomics: every output is written once,
// and the weight gradient is a fixed-order sum (registers -> LDS tree -> one partial row per
// block -> a second pass over the rows), so a replayed graph equals the eager step bit for bit.
#include "layer_dev.h"

namespace damd {
namespace {

// grid-stride launches of at most 8 blocks of 4 waves per CU
constexpr int DW_GRID_CAP = 2048;

__device__ __forceinline__ void fma8(float* acc, const float* a, const float* b) {
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = fmaf(a[e], b[e], acc[e]);
}

// One 8-channel vector of pixel (n, ih, iw) as fp32, zeros when (ih, iw) is outside the image: the
// load itself is unconditional (from the clamped pixel), so a thread's taps are independent loads
// the scheduler can keep in flight together -- behind a branch each tap waits for the one before
// (measured: BENCH.md "Depthwise / separable convolutions").
__device__ __forceinline__ void ld_tap(const uint16_t* __restrict__ p, int n, int ih, int iw, int Hh, int Ww, int cg,
                                       int c8, bool ok, float* f) {
  ok = ok && (unsigned)ih < (unsigned)Hh && (unsigned)iw < (unsigned)Ww;
  const int ihc = min(max(ih, 0), Hh - 1), iwc = min(max(iw, 0), Ww - 1);
  uint4 v = reinterpret_cast<const uint4*>(p)[(((long)n * Hh + ihc) * Ww + iwc) * cg + c8];
  if (!ok) v = uint4{0u, 0u, 0u, 0u};
  unpack8(v, f);
}

// y = bf16(act(sum_{i, j in bounds} x[n, oh*sh - pt + i, ow*sw - pl + j, c] w[i, j, c] + bias[c])):
// fp32, taps in (i, j) order, the bias last, one rounding.  K: a square kernel's size at compile
// time (branch-free unrolled taps), or 0: any ph x pw, a loop with a branch per tap.
template <int K>
__global__ __launch_bounds__(NT) void dwconv_fwd_k(const uint16_t* __restrict__ x, const uint16_t* __restrict__ w,
                                                   const float* __restrict__ bias, int relu, PoolGeo g,
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
    if (K) {
#pragma unroll
      for (int kh = 0; kh < K; ++kh)
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          float v[8], t[8];
          ld_tap(x, n, oh * g.sh - g.pt + kh, ow * g.sw - g.pl + kw, g.H, g.W, cg, c8, true, v);
          unpack8(reinterpret_cast<const uint4*>(w)[(kh * K + kw) * cg + c8], t);
          fma8(acc, v, t);
        }
    } else {
      for (int kh = 0; kh < g.ph; ++kh) {
        const int ih = oh * g.sh - g.pt + kh;
        if ((unsigned)ih >= (unsigned)g.H) continue;
        for (int kw = 0; kw < g.pw; ++kw) {
          const int iw = ow * g.sw - g.pl + kw;
          if ((unsigned)iw >= (unsigned)g.W) continue;
          float v[8], t[8];
          unpack8(reinterpret_cast<const uint4*>(x)[(((long)n * g.H + ih) * g.W + iw) * cg + c8], v);
          unpack8(reinterpret_cast<const uint4*>(w)[(kh * g.pw + kw) * cg + c8], t);
          fma8(acc, v, t);
        }
      }
    }
    if (bias) {
      float b[8];
      ld8f(bias + c8 * 8, b);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += b[e];
    }
    if (relu) {
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaxf(acc[e], 0.f);
    }
    reinterpret_cast<uint4*>(y)[i] = pack8(acc);
  }
}

// dx[n, ih, iw, c] = bf16(sum over the taps (i, j) with (ih + pt - i) = oh * sh, (iw + pl - j) =
// ow * sw, oh in [0, Ho), ow in [0, Wo) of dy[n, oh, ow, c] w[i, j, c]): a gather, one thread per
// input pixel vector, every dx written (zeros where no tap reaches).  K: a square kernel's size at
// compile time, stride 1 -- branch-free unrolled taps in (i, j) order -- or 0: any geometry, a
// loop over the output windows that cover the pixel (at stride 2 most taps reach no output, and
// the loop, which visits only those that do, measured faster than K * K unconditional loads).
template <int K>
__global__ __launch_bounds__(NT) void dwconv_dgrad_k(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ w,
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
    if (K) {
#pragma unroll
      for (int kh = 0; kh < K; ++kh) {
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          float d[8], t[8];
          ld_tap(dy, n, ih + g.pt - kh, iw + g.pl - kw, g.Ho, g.Wo, cg, c8, true, d);  // (stride 1: oh = ih + pt - kh)
          unpack8(reinterpret_cast<const uint4*>(w)[(kh * K + kw) * cg + c8], t);
          fma8(acc, d, t);
        }
      }
      reinterpret_cast<uint4*>(dx)[i] = pack8(acc);
      continue;
    }
    // output rows whose window covers ih: oh*sh - pt <= ih <= oh*sh - pt + ph - 1
    const int ohlo = max(0, (ih + g.pt - g.ph + g.sh) / g.sh), ohhi = min(g.Ho - 1, (ih + g.pt) / g.sh);
    const int owlo = max(0, (iw + g.pl - g.pw + g.sw) / g.sw), owhi = min(g.Wo - 1, (iw + g.pl) / g.sw);
    for (int oh = ohlo; oh <= ohhi; ++oh) {
      const int kh = ih - (oh * g.sh - g.pt);
      if (kh < 0 || kh >= g.ph) continue;
      for (int ow = owlo; ow <= owhi; ++ow) {
        const int kw = iw - (ow * g.sw - g.pl);
        if (kw < 0 || kw >= g.pw) continue;
        float d[8], t[8];
        unpack8(reinterpret_cast<const uint4*>(dy)[(((long)n * g.Ho + oh) * g.Wo + ow) * cg + c8], d);
        unpack8(reinterpret_cast<const uint4*>(w)[(kh * g.pw + kw) * cg + c8], t);
        fma8(acc, d, t);
      }
    }
    reinterpret_cast<uint4*>(dx)[i] = pack8(acc);
  }
}

// Weight gradient, pass 1.  A block owns the output pixels [b * ppb, (b + 1) * ppb) and cgb =
// min(C / 8, NT) channel groups (blockIdx.y picks them); thread t is channel group t % cgb and
// pixel lane t / cgb of NT / cgb lanes, so neighbouring threads read neighbouring channels.
// Per pass over the slab a thread keeps R kernel rows x KW taps x 8 channels in registers
// (R = ph for kernels up to 3 x 3, one kernel row at a time from 4 x 4: no spills); the lanes of a
// channel group then meet in LDS, one tap at a time, in a fixed halving tree, and lane 0
// stores the block's partial into part[b][ph * pw * C].
template <int R, int KW>
__global__ __launch_bounds__(NT) void dwconv_wgrad_k(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy,
                                                     PoolGeo g, long ppb, int cgb, float* __restrict__ part) {
  __shared__ float red[NT][8];
  const int cg = g.C / 8;
  const int lanes = NT / cgb;
  const int cl = threadIdx.x % cgb, lane = threadIdx.x / cgb;
  const int c8 = blockIdx.y * cgb + cl;
  const bool live = lane < lanes && c8 < cg;
  const long P = (long)g.N * g.Ho * g.Wo;
  const long p0 = blockIdx.x * ppb, p1 = min(p0 + ppb, P);
  int top = 1;
  while (top < lanes) top <<= 1;
  float* out = part + (size_t)blockIdx.x * g.ph * g.pw * g.C;
  for (int r0 = 0; r0 < g.ph; r0 += R) {
    float acc[R][KW][8];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < KW; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[r][j][e] = 0.f;
    if (live) {
      for (long p = p0 + lane; p < p1; p += lanes) {
        const int ow = (int)(p % g.Wo);
        const long q = p / g.Wo;
        const int oh = (int)(q % g.Ho);
        const int n = (int)(q / g.Ho);
        float d[8];
        unpack8(reinterpret_cast<const uint4*>(dy)[p * cg + c8], d);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int j = 0; j < KW; ++j) {
            float v[8];
            ld_tap(x, n, oh * g.sh - g.pt + r0 + r, ow * g.sw - g.pl + j, g.H, g.W, cg, c8, true, v);
            fma8(acc[r][j], v, d);
          }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int j = 0; j < KW; ++j) {
        __syncthreads();  // (the previous tap's readers are done)
#pragma unroll
        for (int e = 0; e < 8; ++e) red[threadIdx.x][e] = acc[r][j][e];
        __syncthreads();
        for (int h = top >> 1; h > 0; h >>= 1) {
          if (live && lane < h && lane + h < lanes) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red[threadIdx.x][e] += red[threadIdx.x + h * cgb][e];
          }
          __syncthreads();
        }
        if (live && lane == 0) {
          float* o = out + (size_t)((r0 + r) * KW + j) * g.C + c8 * 8;
          reinterpret_cast<float4*>(o)[0] = *reinterpret_cast<const float4*>(&red[threadIdx.x][0]);
          reinterpret_cast<float4*>(o)[1] = *reinterpret_cast<const float4*>(&red[threadIdx.x][4]);
        }
      }
  }
}

// Weight gradient, pass 2: dw[c] += sum over the T partial rows of part[t][c], in a fixed order.
// A block owns 8 columns (two float4 per row) and 128 row lanes: lane l sums rows l, l + 128, ...
// in order, the lanes meet in an LDS halving tree.  (colsum would sum these rows too, but with
// one block per 64 columns -- 9 blocks for 3 x 3 x 64 -- and every thread walking T / 4 rows.)
constexpr int FIN_Q = 2, FIN_L = NT / FIN_Q;
__global__ __launch_bounds__(NT) void dwconv_wgrad_fin_k(const float* __restrict__ part, int T, int N,
                                                         float* __restrict__ dw) {
  __shared__ float4 red[NT];
  const int q = threadIdx.x % FIN_Q, lane = threadIdx.x / FIN_Q;
  const int col = (blockIdx.x * FIN_Q + q) * 4;
  float4 a{0.f, 0.f, 0.f, 0.f};
  if (col < N)
    for (int t = lane; t < T; t += FIN_L) {
      const float4 v = *reinterpret_cast<const float4*>(part + (size_t)t * N + col);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  red[threadIdx.x] = a;
  __syncthreads();
  for (int h = FIN_L / 2; h > 0; h >>= 1) {
    if (lane < h) {
      const float4 b = red[threadIdx.x + h * FIN_Q];
      float4& r = red[threadIdx.x];
      r.x += b.x; r.y += b.y; r.z += b.z; r.w += b.w;
    }
    __syncthreads();
  }
  if (lane == 0 && col < N) {
    float4 o = *reinterpret_cast<const float4*>(dw + col);
    const float4 r = red[threadIdx.x];
    o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
    *reinterpret_cast<float4*>(dw + col) = o;
  }
}

bool dw_geo_ok(const PoolGeo& g) {
  return g.N > 0 && g.H > 0 && g.W > 0 && g.C > 0 && g.C % 8 == 0 && g.ph > 0 && g.pw > 0 && g.sh > 0 && g.sw > 0 &&
         g.pt >= 0 && g.pl >= 0 && g.pt < g.ph && g.pl < g.pw && g.Ho > 0 && g.Wo > 0 &&
         // every window starts inside the padded image: the last one at or before the last row / column
         (long)(g.Ho - 1) * g.sh - g.pt < g.H && (long)(g.Wo - 1) * g.sw - g.pl < g.W;
}

}  // namespace

hipError_t dwconv_fwd(const uint16_t* x, const uint16_t* w, const float* bias, int relu, const PoolGeo& g,
                      uint16_t* y, hipStream_t s) {
  if (!x || !w || !y || !dw_geo_ok(g)) return hipErrorInvalidValue;
  const dim3 grid(grid_for((long)g.N * g.Ho * g.Wo * g.C / 8, NT, DW_GRID_CAP));
  const int k = g.ph == g.pw ? g.ph : 0;
  auto fn = k == 3 ? dwconv_fwd_k<3> : k == 5 ? dwconv_fwd_k<5> : k == 1 ? dwconv_fwd_k<1> : dwconv_fwd_k<0>;
  hipLaunchKernelGGL(fn, grid, dim3(NT), 0, s, x, w, bias, relu, g, y);
  return hipGetLastError();
}

hipError_t dwconv_dgrad(const uint16_t* dy, const uint16_t* w, const PoolGeo& g, uint16_t* dx, hipStream_t s) {
  if (!dy || !w || !dx || !dw_geo_ok(g)) return hipErrorInvalidValue;
  const dim3 grid(grid_for((long)g.N * g.H * g.W * g.C / 8, NT, DW_GRID_CAP));
  const int k = g.ph == g.pw && g.sh == 1 && g.sw == 1 ? g.ph : 0;
  auto fn = k == 3 ? dwconv_dgrad_k<3> : k == 5 ? dwconv_dgrad_k<5> : k == 1 ? dwconv_dgrad_k<1> : dwconv_dgrad_k<0>;
  hipLaunchKernelGGL(fn, grid, dim3(NT), 0, s, dy, w, g, dx);
  return hipGetLastError();
}

int dwconv_grid_cap() { return DW_GRID_CAP; }

// pixel slabs of the weight gradient: at least 8 output pixels per pixel lane, at most 1024
// blocks (4 per CU)
int dwconv_wgrad_blocks(const PoolGeo& g) {
  const int cgb = g.C / 8 < NT ? g.C / 8 : NT;
  const long P = (long)g.N * g.Ho * g.Wo, per = (long)(NT / cgb) * 8;
  long T = (P + per - 1) / per;
  return (int)(T < 1 ? 1 : T > 1024 ? 1024 : T);
}

hipError_t dwconv_wgrad(const uint16_t* x, const uint16_t* dy, const PoolGeo& g, float* dw, float* ws, hipStream_t s) {
  if (!x || !dy || !dw || !ws || !dw_geo_ok(g) || g.ph != g.pw) return hipErrorInvalidValue;
  if (g.ph > 7) return hipErrorInvalidValue;
  const int cg = g.C / 8, cgb = cg < NT ? cg : NT;
  const int T = dwconv_wgrad_blocks(g), KK = g.ph * g.pw;
  const long P = (long)g.N * g.Ho * g.Wo, ppb = (P + T - 1) / T;
  const dim3 grid(T, (cg + cgb - 1) / cgb);
#define DW_WGRAD(R_, KW_) \
  hipLaunchKernelGGL((dwconv_wgrad_k<R_, KW_>), grid, dim3(NT), 0, s, x, dy, g, ppb, cgb, ws)
  switch (g.ph) {
    case 1: DW_WGRAD(1, 1); break;
    case 2: DW_WGRAD(2, 2); break;
    case 3: DW_WGRAD(3, 3); break;
    case 4: DW_WGRAD(1, 4); break;
    case 5: DW_WGRAD(1, 5); break;
    case 6: DW_WGRAD(1, 6); break;
    default: DW_WGRAD(1, 7); break;
  }
#undef DW_WGRAD
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // pass 2: dw += the T partial rows
  const int N = KK * g.C;
  hipLaunchKernelGGL(dwconv_wgrad_fin_k, dim3((N / 4 + FIN_Q - 1) / FIN_Q), dim3(NT), 0, s, ws, T, N, dw);
  return hipGetLastError();
}

}  // namespace damd
