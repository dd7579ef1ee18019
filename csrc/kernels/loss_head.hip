// The model's head on the generic path: softmax cross-entropy against sparse labels or dense
// target rows (loss, accuracy, dlogits and optionally the logits layer's bias gradient in
// one launch), the inference outputs (logits / softmax rows stored at the device cursor),
// and the column sums that form bias gradients.  Every batch reduction here runs in a fixed
// order -- per-row results, then the last block to arrive (damd_common.h last_arriver) adds
// them up -- never by float atomics, so replays and graph / eager runs give the same bits.
#include "layer_dev.h"

namespace damd {
namespace {

// Column sums in a fixed order (bias gradients; no float atomics).  grid (ceil(N/64),
// splits), 4 row phases per block: split y sums rows y*4+ph, y*4+ph + 4*splits, ...; one
// split adds straight into out[n], several write slab[y][n] and colsum_fin_k adds the
// slabs in split order.
__global__ __launch_bounds__(NT) void colsum_k(const void* x, int x_f32, int M, int N, int ld, float* out,
                                               float* slab) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + cl;
  float a = 0.f;
  if (n < N)
    for (int m = blockIdx.y * 4 + ph; m < M; m += gridDim.y * 4)
      a += x_f32 ? ((const float*)x)[(size_t)m * ld + n] : bf2f(((const uint16_t*)x)[(size_t)m * ld + n]);
  red[ph][cl] = a;
  __syncthreads();
  if (ph == 0 && n < N) {
    const float v = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
    if (gridDim.y == 1) out[n] += v;
    else slab[(size_t)blockIdx.y * N + n] = v;
  }
}
__global__ __launch_bounds__(NT) void colsum_fin_k(const float* slab, int splits, int N, float* out) {
  const int n = blockIdx.x * NT + threadIdx.x;
  if (n >= N) return;
  float a = 0.f;
  for (int y = 0; y < splits; ++y) a += slab[(size_t)y * N + n];
  out[n] += a;
}

// ---- loss ------------------------------------------------------------------------------------
// Rows with label < 0 (past the end of the dataset in a short final batch) get a zero
// gradient and no loss / metric contribution.  With ctrl != nullptr the gradient scale is
// 1 / (rows of this global batch that exist): Keras' SUM_OVER_BATCH_SIZE on the real
// final batch; benchmark wrap mode (ctrl->wrap > 0) always has full batches.
// One block per row; the row is read from memory once (up to 4 values per thread held in
// registers) and reduced by wave shuffles plus one LDS exchange per quantity.  The first
// version re-read the row for the max, the exponent sum and the output, and reduced each
// by an 8-level LDS tree (17 barriers per row, 30 more in the last block): 9.8 us for the
// ResNet-18 head (64 x 1000) -- the 1000-class logits of 64 rows.
constexpr int SX_KPT = 4, SX_BK = 1024;
__device__ __forceinline__ void sx_better(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }  // max, ties -> smallest index
}
__device__ __forceinline__ void sx_better_sel(float& v, int& i, float ov, int oi) {
  const bool take = (ov > v) | ((ov == v) & (oi < i));  // sx_better as selects: no branch
  v = take ? ov : v;
  i = take ? oi : i;
}
// The end of both loss kernels: the batch sums and the logits layer's bias gradient.
// Every thread of every block calls it (last_arriver holds barriers).
__device__ __forceinline__ void sx_tail(float row_loss, float row_corr, float row_valid, int K, int ld,
                                        const uint16_t* dl, float* tail, float* rows, float* bias_grad) {
  __shared__ float wtail[3][SX_NW];
  __shared__ int last;
  const int b = blockIdx.x, t = threadIdx.x, B = gridDim.x, lane = t & 63, w = t >> 6;
  // the batch sums in a fixed order (no float atomics: replays and graph / eager runs give
  // the same bits): every row stores (loss, correct, valid), the last block to arrive adds
  // them up (fixed shuffle tree + fixed wave order) and re-arms the arrival counter rows[3 B]
  if (t == 0) {
    rows[3 * b] = row_loss;
    rows[3 * b + 1] = row_corr;
    rows[3 * b + 2] = row_valid;
  }
  int* counter = reinterpret_cast<int*>(rows + 3 * B);
  if (!last_arriver(counter, B, &last)) return;
  float a[3] = {0.f, 0.f, 0.f};
  for (int r = t; r < B; r += NT)
#pragma unroll
    for (int q = 0; q < 3; ++q) a[q] += rows[3 * r + q];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    a[q] = sx_wave_sum(a[q]);
    if (lane == 0) wtail[q][w] = a[q];
  }
  __syncthreads();
  if (t < 3) {
    float v = wtail[t][0];
#pragma unroll
    for (int u = 1; u < SX_NW; ++u) v += wtail[t][u];
    tail[t] += v;
  }
  if (t == 0) *counter = 0;
  if (bias_grad) {
    // the logits layer's bias gradient from the stored dl rows (every block's, acquired by
    // last_arriver), in colsum_k's one-split order: 4 row phases each summed in row order,
    // then (p0 + p1) + (p2 + p3), added to the gradient -- the same bits as its launch.
    // Work item = (phase, 8 columns): 16-byte loads of 8 rows in flight at a time, the
    // phase sums meet in LDS (a thread per column walking the rows one load at a time took
    // the launch from 7.5 to 66 us)
    __shared__ float bph[4][SX_BK];
    if (K <= SX_BK && ld % 8 == 0) {
      const int ng = (K + 7) / 8;
      for (int wi = t; wi < 4 * ng; wi += NT) {
        const int q = wi / ng, g = wi - q * ng;
        float s8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int m0 = q; m0 < B; m0 += 32) {
          uint4 v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int m = m0 + 4 * u;
            v[u] = m < B ? *reinterpret_cast<const uint4*>(dl + (size_t)m * ld + 8 * g) : uint4{0u, 0u, 0u, 0u};
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            if (m0 + 4 * u >= B) break;
            const uint32_t w4[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              s8[2 * e] += __uint_as_float(w4[e] << 16);
              s8[2 * e + 1] += __uint_as_float(w4[e] & 0xffff0000u);
            }
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) bph[q][8 * g + e] = s8[e];
      }
      __syncthreads();
      for (int k = t; k < K; k += NT) bias_grad[k] += (bph[0][k] + bph[1][k]) + (bph[2][k] + bph[3][k]);
    } else {
      for (int k = t; k < K; k += NT) {
        float ph[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          for (int m = q; m < B; m += 4) ph[q] += bf2f(dl[(size_t)m * ld + k]);
        bias_grad[k] += (ph[0] + ph[1]) + (ph[2] + ph[3]);
      }
    }
  }
}

// W: a per-row weight (Keras sample / class weights) multiplies the row's gradient and loss,
// not its correct / valid counts: weights[b] without ctrl, else the weight of the sample at
// the device cursor, weights[cursor * global_batch + row0 + b] (modulo nsamples in wrap
// mode) -- the row softmax_xent_dense_k reads its targets from.  A row with label < 0 does
// not read the array.  The weights pointer is an argument of the W = true instantiation
// alone (Wt = const float*): W = false (no Wt) keeps the argument list, the kernarg layout
// and the instruction stream of the unweighted kernel as it was before there were weights.
__device__ __forceinline__ const float* sx_weights() { return nullptr; }
__device__ __forceinline__ const float* sx_weights(const float* w) { return w; }
template <bool W, typename... Wt>
__global__ __launch_bounds__(NT) void softmax_xent_k(const float* __restrict__ logits, int ld,
                                                     const int32_t* __restrict__ labels, int K, float scale,
                                                     const Ctrl* __restrict__ ctrl, uint16_t* __restrict__ dl,
                                                     float* tail, float* rows, float* bias_grad, Wt... weights) {
  __shared__ float wmax[SX_NW], wsum[SX_NW];
  __shared__ int widx[SX_NW];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int y = labels[b];
  float row_loss = 0.f, row_corr = 0.f;
  if (y < 0) {
    for (int k = t; k < K; k += NT) dl[(size_t)b * ld + k] = 0;
  } else {
    [[maybe_unused]] long row = b;
    if (ctrl) {
      const int gb = ctrl->global_batch;
      const int left = ctrl->nsamples - ctrl->cursor * gb;
      scale = 1.f / (float)(ctrl->wrap > 0 ? gb : max(1, min(gb, left)));
      if constexpr (W) {
        const long base = (long)ctrl->cursor * gb + ctrl->row0;
        row = ctrl->wrap > 0 ? (base + b) % ctrl->nsamples : base + b;
      }
    }
    [[maybe_unused]] float wt = 1.f;
    if constexpr (W) {
      wt = sx_weights(weights...)[row];
      scale *= wt;
    }
    const float* z = logits + (size_t)b * ld;
    const bool reg = K <= SX_KPT * NT;  // the row fits the registers
    float zr[SX_KPT];
    float mx = -INFINITY;
    int mi = 0x7fffffff;
    if (reg) {
#pragma unroll
      for (int i = 0; i < SX_KPT; ++i) zr[i] = t + i * NT < K ? z[t + i * NT] : -INFINITY;
#pragma unroll
      for (int i = 0; i < SX_KPT; ++i)
        if (t + i * NT < K && zr[i] > mx) { mx = zr[i]; mi = t + i * NT; }
    } else {
      for (int k = t; k < K; k += NT) {
        const float v = z[k];
        if (v > mx) { mx = v; mi = k; }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sx_better(mx, mi, __shfl_xor(mx, o), __shfl_xor(mi, o));
    if (lane == 0) { wmax[w] = mx; widx[w] = mi; }
    __syncthreads();
    float zmax = wmax[0];
    int amax = widx[0];
#pragma unroll
    for (int v = 1; v < SX_NW; ++v) sx_better(zmax, amax, wmax[v], widx[v]);
    float se = 0.f;
    if (reg) {
#pragma unroll
      for (int i = 0; i < SX_KPT; ++i) {
        zr[i] = t + i * NT < K ? __expf(zr[i] - zmax) : 0.f;
        se += zr[i];
      }
    } else {
      for (int k = t; k < K; k += NT) se += __expf(z[k] - zmax);
    }
    se = sx_wave_sum(se);
    if (lane == 0) wsum[w] = se;
    __syncthreads();
    float sum = wsum[0];
#pragma unroll
    for (int v = 1; v < SX_NW; ++v) sum += wsum[v];
    const float inv = 1.f / sum;
    if (reg) {
#pragma unroll
      for (int i = 0; i < SX_KPT; ++i) {
        const int k = t + i * NT;
        if (k < K) dl[(size_t)b * ld + k] = f2bf((zr[i] * inv - (k == y ? 1.f : 0.f)) * scale);
      }
    } else {
      for (int k = t; k < K; k += NT) {
        const float p = __expf(z[k] - zmax) * inv;
        dl[(size_t)b * ld + k] = f2bf((p - (k == y ? 1.f : 0.f)) * scale);
      }
    }
    row_loss = logf(sum) + zmax - z[y];
    if constexpr (W) row_loss *= wt;
    row_corr = amax == y ? 1.f : 0.f;
  }
  sx_tail(row_loss, row_corr, y < 0 ? 0.f : 1.f, K, ld, dl, tail, rows, bias_grad);
}
template __global__ void softmax_xent_k<false>(const float* __restrict__, int, const int32_t* __restrict__, int, float,
                                               const Ctrl* __restrict__, uint16_t* __restrict__, float*, float*,
                                               float*);

// Softmax cross-entropy against dense fp32 target rows (one-hot / soft targets) with label
// smoothing: y' = y (1 - eps) + eps / K, S = sum y', loss = S lse - sum y' z, dlogits =
// (p S - y') scale (S: targets need not sum to 1), correct = argmax z == argmax y, both
// ties to the smallest index.  The structure of softmax_xent_k; the targets ride along
// with the logits (both loads issued together), and the first LDS exchange carries the
// two argmaxes, S and the dot product at once, so the row costs the same two barriers.
// With ctrl the block finds its target row as gather_batch_k finds the input row (the
// epoch-ordered [n][K] targets are read in place), else targets are indexed by the block.
// labels (optional): labels[b] < 0 marks a row past the end of the data.
// W: weights[row] of that same row multiplies the gradient and the loss (softmax_xent_k,
// instantiated the same way).
template <bool W, typename... Wt>
__global__ __launch_bounds__(NT) void softmax_xent_dense_k(const float* __restrict__ logits, int ld,
                                                           const int32_t* __restrict__ labels,
                                                           const float* __restrict__ targets, int K, float eps,
                                                           float scale, const Ctrl* __restrict__ ctrl,
                                                           uint16_t* __restrict__ dl, float* tail, float* rows,
                                                           float* bias_grad, Wt... weights) {
  __shared__ float wmax[SX_NW], wymax[SX_NW], wS[SX_NW], wdot[SX_NW], wsum[SX_NW];
  __shared__ int widx[SX_NW], wyidx[SX_NW];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const bool valid = labels == nullptr || labels[b] >= 0;
  float row_loss = 0.f, row_corr = 0.f;
  if (!valid) {
    for (int k = t; k < K; k += NT) dl[(size_t)b * ld + k] = 0;
  } else {
    long row = b;
    if (ctrl) {
      const int gb = ctrl->global_batch;
      const int left = ctrl->nsamples - ctrl->cursor * gb;
      scale = 1.f / (float)(ctrl->wrap > 0 ? gb : max(1, min(gb, left)));
      const long base = (long)ctrl->cursor * gb + ctrl->row0;
      row = ctrl->wrap > 0 ? (base + b) % ctrl->nsamples : base + b;
    }
    [[maybe_unused]] float wt = 1.f;
    if constexpr (W) {
      wt = sx_weights(weights...)[row];
      scale *= wt;
    }
    const float* z = logits + (size_t)b * ld;
    const float* yt = targets + (size_t)row * K;
    const float keep = 1.f - eps, uni = eps / (float)K;
    const bool reg = K <= SX_KPT * NT;  // the row fits the registers
    float zr[SX_KPT], yr[SX_KPT];
    float mx = -INFINITY, my = -INFINITY, S = 0.f, dot = 0.f;
    int mi = 0x7fffffff, yi = 0x7fffffff;
    if (reg) {
#pragma unroll
      for (int i = 0; i < SX_KPT; ++i) {
        const bool in = t + i * NT < K;
        zr[i] = in ? z[t + i * NT] : -INFINITY;
        yr[i] = in ? yt[t + i * NT] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < SX_KPT; ++i) {
        if (t + i * NT >= K) continue;
        if (zr[i] > mx) { mx = zr[i]; mi = t + i * NT; }
        if (yr[i] > my) { my = yr[i]; yi = t + i * NT; }
        yr[i] = yr[i] * keep + uni;
        S += yr[i];
        dot += yr[i] * zr[i];
      }
    } else {
      for (int k = t; k < K; k += NT) {
        const float v = z[k], u = yt[k];
        if (v > mx) { mx = v; mi = k; }
        if (u > my) { my = u; yi = k; }
        const float ys = u * keep + uni;
        S += ys;
        dot += ys * v;
      }
    }
    // the four reductions level by level: a level's six shuffles go out together and the
    // argmaxes are selects (sx_better's branches made the compiler run the chains one after
    // the other, 12 dependent shuffle round trips more than softmax_xent_k: +1.07 us at
    // 64 x 1000)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(mx, o), oy = __shfl_xor(my, o), oS = __shfl_xor(S, o), od = __shfl_xor(dot, o);
      const int oi = __shfl_xor(mi, o), oyi = __shfl_xor(yi, o);
      sx_better_sel(mx, mi, ov, oi);
      sx_better_sel(my, yi, oy, oyi);
      S += oS;
      dot += od;
    }
    if (lane == 0) { wmax[w] = mx; widx[w] = mi; wymax[w] = my; wyidx[w] = yi; wS[w] = S; wdot[w] = dot; }
    __syncthreads();
    float zmax = wmax[0], ymax = wymax[0];
    int amax = widx[0], ymaxi = wyidx[0];
    S = wS[0];
    dot = wdot[0];
#pragma unroll
    for (int v = 1; v < SX_NW; ++v) {
      sx_better_sel(zmax, amax, wmax[v], widx[v]);
      sx_better_sel(ymax, ymaxi, wymax[v], wyidx[v]);
      S += wS[v];
      dot += wdot[v];
    }
    float se = 0.f;
    if (reg) {
#pragma unroll
      for (int i = 0; i < SX_KPT; ++i) {
        zr[i] = t + i * NT < K ? __expf(zr[i] - zmax) : 0.f;
        se += zr[i];
      }
    } else {
      for (int k = t; k < K; k += NT) se += __expf(z[k] - zmax);
    }
    se = sx_wave_sum(se);
    if (lane == 0) wsum[w] = se;
    __syncthreads();
    float sum = wsum[0];
#pragma unroll
    for (int v = 1; v < SX_NW; ++v) sum += wsum[v];
    const float inv = 1.f / sum;
    if (reg) {
#pragma unroll
      for (int i = 0; i < SX_KPT; ++i) {
        const int k = t + i * NT;
        if (k < K) dl[(size_t)b * ld + k] = f2bf((zr[i] * inv * S - yr[i]) * scale);
      }
    } else {
      for (int k = t; k < K; k += NT) {
        const float p = __expf(z[k] - zmax) * inv;
        dl[(size_t)b * ld + k] = f2bf((p * S - (yt[k] * keep + uni)) * scale);
      }
    }
    row_loss = S * (logf(sum) + zmax) - dot;
    if constexpr (W) row_loss *= wt;
    row_corr = amax == ymaxi ? 1.f : 0.f;
  }
  sx_tail(row_loss, row_corr, valid ? 1.f : 0.f, K, ld, dl, tail, rows, bias_grad);
}
template __global__ void softmax_xent_dense_k<false>(const float* __restrict__, int, const int32_t* __restrict__,
                                                     const float* __restrict__, int, float, float,
                                                     const Ctrl* __restrict__, uint16_t* __restrict__, float*, float*,
                                                     float*);

// ---- inference outputs ---------------------------------------------------------------------
// logits rows of this step -> out[global row][K] (rows past the end of the data dropped);
// the row base comes from the device cursor, so a captured graph replays across batches
__global__ __launch_bounds__(NT) void logits_store_k(const float* __restrict__ logits, int ld, int K, int B,
                                                     const Ctrl* __restrict__ ctrl, float* __restrict__ out) {
  const long base = (long)ctrl->cursor * ctrl->global_batch + ctrl->row0;
  const long n = ctrl->nsamples;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < (long)B * K; i += (long)gridDim.x * NT) {
    const int r = (int)(i / K), k = (int)(i % K);
    if (base + r < n) out[(base + r) * K + k] = logits[(long)r * ld + k];
  }
}

// logits_store_k for a model whose output is a softmax: out[global row][K] = softmax of the
// step's logits row.  One block per row (the row held in registers up to SX_KPT * NT
// columns, re-read beyond), rows past the end of the data dropped.
__global__ __launch_bounds__(NT) void softmax_store_k(const float* __restrict__ logits, int ld, int K,
                                                      const Ctrl* __restrict__ ctrl, float* __restrict__ out) {
  __shared__ float wmax[SX_NW], wsum[SX_NW];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long r = (long)ctrl->cursor * ctrl->global_batch + ctrl->row0 + b;
  if (r >= ctrl->nsamples) return;  // the whole block: no barrier is left waiting
  const float* z = logits + (size_t)b * ld;
  float* o = out + r * K;
  const bool reg = K <= SX_KPT * NT;
  float zr[SX_KPT];
  float mx = -INFINITY;
  if (reg) {
#pragma unroll
    for (int i = 0; i < SX_KPT; ++i) {
      zr[i] = t + i * NT < K ? z[t + i * NT] : -INFINITY;
      mx = fmaxf(mx, zr[i]);
    }
  } else {
    for (int k = t; k < K; k += NT) mx = fmaxf(mx, z[k]);
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s));
  if (lane == 0) wmax[w] = mx;
  __syncthreads();
  float zmax = wmax[0];
#pragma unroll
  for (int v = 1; v < SX_NW; ++v) zmax = fmaxf(zmax, wmax[v]);
  float se = 0.f;
  if (reg) {
#pragma unroll
    for (int i = 0; i < SX_KPT; ++i) {
      zr[i] = t + i * NT < K ? __expf(zr[i] - zmax) : 0.f;
      se += zr[i];
    }
  } else {
    for (int k = t; k < K; k += NT) se += __expf(z[k] - zmax);
  }
  se = sx_wave_sum(se);
  if (lane == 0) wsum[w] = se;
  __syncthreads();
  float sum = wsum[0];
#pragma unroll
  for (int v = 1; v < SX_NW; ++v) sum += wsum[v];
  const float inv = 1.f / sum;
  if (reg) {
#pragma unroll
    for (int i = 0; i < SX_KPT; ++i)
      if (t + i * NT < K) o[t + i * NT] = zr[i] * inv;
  } else {
    for (int k = t; k < K; k += NT) o[k] = __expf(z[k] - zmax) * inv;
  }
}

// ---- the weighted loss kernels ---------------------------------------------------------------
template __global__ void softmax_xent_k<true, const float*>(const float* __restrict__, int,
                                                            const int32_t* __restrict__, int, float,
                                                            const Ctrl* __restrict__, uint16_t* __restrict__, float*,
                                                            float*, float*, const float*);
template __global__ void softmax_xent_dense_k<true, const float*>(const float* __restrict__, int,
                                                                  const int32_t* __restrict__,
                                                                  const float* __restrict__, int, float, float,
                                                                  const Ctrl* __restrict__, uint16_t* __restrict__,
                                                                  float*, float*, float*, const float*);

}  // namespace

int colsum_splits(int M, int N) {
  // one pass while the column tiles alone give the chip enough blocks or M is short
  if (M <= 4096 || (N + 63) / 64 >= 64) return 1;
  int splits = (M + 1023) / 1024;
  return splits > 64 ? 64 : splits;
}
hipError_t colsum(const void* x, int x_f32, int M, int N, int ld, float* out, float* ws, hipStream_t s) {
  const int splits = colsum_splits(M, N);
  if (splits > 1 && !ws) return hipErrorInvalidValue;
  hipLaunchKernelGGL(colsum_k, dim3((N + 63) / 64, splits), dim3(NT), 0, s, x, x_f32, M, N, ld, out, ws);
  if (splits > 1) hipLaunchKernelGGL(colsum_fin_k, dim3((N + NT - 1) / NT), dim3(NT), 0, s, ws, splits, N, out);
  return hipGetLastError();
}

hipError_t softmax_xent(const float* logits, int ld, const int32_t* labels, int B, int K, float scale, const Ctrl* ctrl,
                        uint16_t* dlogits, float* tail, float* rows, hipStream_t s, float* bias_grad,
                        const float* weights) {
  if (!rows || B < 1) return hipErrorInvalidValue;
  if (bias_grad && colsum_splits(B, K) != 1) return hipErrorInvalidValue;  // the fold keeps colsum's order
  if (weights)
    hipLaunchKernelGGL((softmax_xent_k<true, const float*>), dim3(B), dim3(NT), 0, s, logits, ld, labels, K, scale,
                       ctrl, dlogits, tail, rows, bias_grad, weights);
  else
    hipLaunchKernelGGL(softmax_xent_k<false>, dim3(B), dim3(NT), 0, s, logits, ld, labels, K, scale, ctrl, dlogits,
                       tail, rows, bias_grad);
  return hipGetLastError();
}

hipError_t softmax_xent_dense(const float* logits, int ld, const int32_t* labels, const float* targets, int B, int K,
                              float label_smoothing, float scale, const Ctrl* ctrl, uint16_t* dlogits, float* tail,
                              float* rows, hipStream_t s, float* bias_grad, const float* weights) {
  if (!rows || !targets || B < 1 || K < 1 || K > ld) return hipErrorInvalidValue;
  if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return hipErrorInvalidValue;
  if (ctrl && !labels) return hipErrorInvalidValue;  // the step's row validity comes from gather_batch
  if (bias_grad && colsum_splits(B, K) != 1) return hipErrorInvalidValue;  // the fold keeps colsum's order
  if (weights)
    hipLaunchKernelGGL((softmax_xent_dense_k<true, const float*>), dim3(B), dim3(NT), 0, s, logits, ld, labels,
                       targets, K, label_smoothing, scale, ctrl, dlogits, tail, rows, bias_grad, weights);
  else
    hipLaunchKernelGGL(softmax_xent_dense_k<false>, dim3(B), dim3(NT), 0, s, logits, ld, labels, targets, K,
                       label_smoothing, scale, ctrl, dlogits, tail, rows, bias_grad);
  return hipGetLastError();
}

hipError_t logits_store(const float* logits, int ld, int K, int B, const Ctrl* ctrl, float* out, hipStream_t s) {
  if (K > ld || K < 1 || B < 1 || !ctrl) return hipErrorInvalidValue;
  hipLaunchKernelGGL(logits_store_k, dim3(grid_for((long)B * K)), dim3(NT), 0, s, logits, ld, K, B, ctrl, out);
  return hipGetLastError();
}

hipError_t softmax_store(const float* logits, int ld, int K, int B, const Ctrl* ctrl, float* out, hipStream_t s) {
  if (K > ld || K < 1 || B < 1 || !ctrl) return hipErrorInvalidValue;
  hipLaunchKernelGGL(softmax_store_k, dim3(B), dim3(NT), 0, s, logits, ld, K, ctrl, out);
  return hipGetLastError();
}

}  // namespace damd
