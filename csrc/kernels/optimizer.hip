// The optimizer tail of a training step on the flat fp32 master buffer (+ bf16 shadow read by
// the MFMA GEMMs): the flat multi-tensor SGD, the graph-captured step kernels (sgd_step,
// opt_step: SGD / Adam / RMSprop with weight regularizers, gradient clipping and on-device
// learning-rate schedules), the regularizer penalty, the clipping norm, and the inference
// step's bookkeeping (step_fold).  The reductions (reg_penalty, grad_norm) run in a fixed
// order with a last-arriver block, no float atomics: two launches give the same bits.
//
// opt_step_k and the helpers it is built from stand outside the anonymous namespace: the
// kernel keeps its external damd::opt_step_k<...> symbols.
#include "layer_dev.h"

namespace damd {

// Keras optimizer_v2 update rules on the flat fp32 master buffer (+ bf16 shadow): the
// native-engine counterpart of keras/optimizers.py apply_flat.  lr from ctrl (a new rate
// needs no re-capture) or from a schedule descriptor (SCHED, lr_eval below); Adam's step
// t = ctrl->cur3, written by gather_batch at the start of the step (no block of this kernel
// reads a ctrl field this kernel writes: under SCHED the bookkeeping thread stores lr, which
// no launch then reads).
//
// Weight regularizers (REG): a segment table, one row (offset, size, l1 bits, l2 bits) per
// regularized variable, sorted by offset; offsets index the engine's whole flat buffer and
// element 0 of this launch is element `lo` of it (per-bucket launches).  The block stages
// the table into LDS once; each thread finds the row of its element by a binary search
// there (the row found last is tried first) and uses g = G[i] + (2 l2 w + l1 sign(w)),
// sign(0) = 0, formed from the fp32 master AFTER the all-reduce: counted once whatever the
// world size, exact under bf16 gradient buckets.  REG = false is the kernel without any of it.
struct RegSeg {
  int off, end;  // [off, end) of the flat buffer; off > end: none
  float l1, l2;
};
// the row covering element i of a table of nreg rows (LDS), or an empty one
__device__ __forceinline__ RegSeg reg_find(const int4* tab, int nreg, long i) {
  int a = 0, b = nreg;  // the last row with offset <= i is a - 1
  while (a < b) {
    const int m = (a + b) >> 1;
    if ((long)tab[m].x <= i) a = m + 1; else b = m;
  }
  RegSeg r{1, 0, 0.f, 0.f};
  if (a > 0) {
    const int4 q = tab[a - 1];
    if (i < (long)q.x + q.y) r = RegSeg{q.x, q.x + q.y, __int_as_float(q.z), __int_as_float(q.w)};
  }
  return r;
}
__device__ __forceinline__ void reg_stage(int4* lds, const int4* tab, int nreg) {
  for (int r = threadIdx.x; r < nreg; r += NT) lds[r] = tab[r];
  __syncthreads();
}

// Gradient clipping (CLIP; keras/optimizers.py), applied to the regularized g before the
// update rule: CLIP_VALUE clamps g to [-clipc, clipc] (a NaN stays a NaN); CLIP_GLOBAL uses
// g * scales[0]; CLIP_VAR uses g * scales[row], row = the element's row of the table, which
// then lists EVERY variable (zero coefficients where there is no regularizer) so that the
// row index also indexes grad_norm's scale array.  A scale of exactly 1.0f leaves g's bits
// alone.  CLIP_NONE is the kernel without any of it (no load, no LDS beyond REG's).
enum : int { CLIP_NONE = 0, CLIP_VALUE = 1, CLIP_VAR = 2, CLIP_GLOBAL = 3 };
// the index of the row covering element i of a table of nreg rows (LDS), or -1
__device__ __forceinline__ int reg_find_row(const int4* tab, int nreg, long i) {
  int a = 0, b = nreg;  // reg_find's search: the last row with offset <= i is a - 1
  while (a < b) {
    const int m = (a + b) >> 1;
    if ((long)tab[m].x <= i) a = m + 1; else b = m;
  }
  return (a > 0 && i < (long)tab[a - 1].x + tab[a - 1].y) ? a - 1 : -1;
}

// A Keras learning-rate schedule (SCHED; keras/schedules.py) at `step`, the optimizer's
// iterations before this update: fp32 values, integer step logic -- p, s, d, the boundary
// search and the warm-up branch are exact, so a boundary step never lands on the wrong side
// through rounding.  q is a kernel argument (scalar registers): every index below is a
// compile-time constant after unrolling, every branch wave-uniform.  ops/reference.py
// lr_schedule32 performs the same operations in numpy.float32.
__device__ __forceinline__ float lr_eval(const LrSched& q, int step) {
  const int ds = q.decay_steps;
  switch (q.kind) {
    case LR_EXPONENTIAL:
    case LR_INVERSE_TIME: {
      const float p = (q.flags & 1) ? (float)(step / ds) : (float)step / (float)ds;
      return q.kind == LR_EXPONENTIAL ? q.init * powf(q.a, p) : q.init / (1.f + q.a * p);
    }
    case LR_POLYNOMIAL: {
      long s = step < ds ? step : ds, d = ds;
      if (q.flags & 1) {
        const long m = ((long)step + ds - 1) / ds;  // ceil(step / decay_steps)
        s = step;
        d = (long)ds * (m > 1 ? m : 1);
      }
      return (q.init - q.a) * powf(1.f - (float)s / (float)d, q.b) + q.a;
    }
    case LR_PIECEWISE: {
      float v = q.values[0];
#pragma unroll
      for (int i = 0; i < LR_MAX_BOUNDS; ++i)
        if (i < q.nbounds && step > q.bounds[i]) v = q.values[i + 1];
      return v;
    }
    default: {  // LR_COSINE
      float init = q.init;
      if (q.flags & 1) {
        if (step < q.warmup_steps) return q.init + (q.b - q.init) * (float)step / (float)q.warmup_steps;
        init = q.b;
        step -= q.warmup_steps;
      }
      const int s = step < ds ? step : ds;
      const float c = cosf(3.14159265358979323846f * (float)s / (float)ds);
      return init * ((1.f - q.a) * 0.5f * (1.f + c) + q.a);
    }
  }
}

template <bool REG, int CLIP, bool SCHED>
__global__ __launch_bounds__(NT) void opt_step_k(float* __restrict__ P, const float* __restrict__ G,
                                                 float* __restrict__ S0, float* __restrict__ S1,
                                                 float* __restrict__ S2, uint16_t* __restrict__ Pb, long n,
                                                 Ctrl* ctrl, const float* tail, OptArgs o, int book,
                                                 const int4* reg, int nreg, long lo, float clipc,
                                                 const float* __restrict__ scales, LrSched sched) {
  extern __shared__ __attribute__((aligned(16))) int4 reg_lds[];
  RegSeg seg{1, 0, 0.f, 0.f};
  if constexpr (REG || CLIP == CLIP_VAR) reg_stage(reg_lds, reg, nreg);
  float gscale = 1.f;  // CLIP_GLOBAL: the one scale; CLIP_VAR: the scale of seg's row
  if constexpr (CLIP == CLIP_GLOBAL) gscale = scales[0];
  const int t = ctrl->cur3;
  float lr;
  if constexpr (SCHED) lr = lr_eval(sched, t > 1 ? t - 1 : 0);
  else lr = ctrl->lr;
  float lr_t = lr;
  if (o.kind == 1) lr_t = lr * sqrtf(1.f - powf(o.b2, (float)t)) / (1.f - powf(o.b1, (float)t));
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
    float g = G[i];
    float w = P[i];
    if constexpr (CLIP == CLIP_VAR) {
      const long a = lo + i;
      if (a < seg.off || a >= seg.end) {
        const int row = reg_find_row(reg_lds, nreg, a);
        seg = RegSeg{1, 0, 0.f, 0.f};
        gscale = 1.f;  // padding between variables: g = 0, no row
        if (row >= 0) {
          const int4 q = reg_lds[row];
          seg = RegSeg{q.x, q.x + q.y, __int_as_float(q.z), __int_as_float(q.w)};
          gscale = scales[row];
        }
      }
      if (a >= seg.off && a < seg.end && (seg.l1 != 0.f || seg.l2 != 0.f)) {
        const float sgn = (float)((w > 0.f) - (w < 0.f));
        g += fmaf(2.f * seg.l2, w, seg.l1 * sgn);
      }
    } else if constexpr (REG) {
      const long a = lo + i;
      if (a < seg.off || a >= seg.end) seg = reg_find(reg_lds, nreg, a);
      if (a >= seg.off && a < seg.end) {
        const float sgn = (float)((w > 0.f) - (w < 0.f));
        g += fmaf(2.f * seg.l2, w, seg.l1 * sgn);
      }
    }
    if constexpr (CLIP == CLIP_VALUE) g = g < -clipc ? -clipc : (g > clipc ? clipc : g);
    if constexpr (CLIP == CLIP_VAR || CLIP == CLIP_GLOBAL) g *= gscale;
    if (o.kind == 1) {  // Adam (S0 m, S1 v, S2 vhat)
      const float m = o.b1 * S0[i] + (1.f - o.b1) * g;
      const float v = o.b2 * S1[i] + (1.f - o.b2) * g * g;
      S0[i] = m;
      S1[i] = v;
      float d = v;
      if (o.flag) {
        d = fmaxf(S2[i], v);
        S2[i] = d;
      }
      w -= lr_t * (m / (sqrtf(d) + o.eps));
    } else if (o.kind == 2) {  // RMSprop (S0 rms, S1 momentum, S2 mg)
      const float ms = o.rho * S0[i] + (1.f - o.rho) * g * g;
      S0[i] = ms;
      float den = ms;
      if (o.flag) {
        const float mg = o.rho * S2[i] + (1.f - o.rho) * g;
        S2[i] = mg;
        den = ms - mg * mg;
      }
      const float upd = g / (sqrtf(den) + o.eps) * lr;
      if (o.mom != 0.f) {
        const float mo = o.mom * S1[i] + upd;
        S1[i] = mo;
        w -= mo;
      } else {
        w -= upd;
      }
    } else {  // SGD (S0 momentum)
      float wn, vn;
      sgd_update(w, g, o.mom != 0.f ? S0[i] : 0.f, lr, o.mom, o.flag, wn, vn);
      if (o.mom != 0.f) S0[i] = vn;
      w = wn;
    }
    P[i] = w;
    Pb[i] = f2bf(w);
  }
  // the step's bookkeeping, once per step: by the launch covering the metric tail's bucket
  // when the update is split per gradient bucket (native_graph bucket_opt), else by the
  // single launch.  (The per-bucket launches only READ ctrl's lr / cur3.)
  if (book && blockIdx.x == 0 && threadIdx.x == 0) {
    ctrl->acc_loss += tail[0];
    ctrl->acc_correct += tail[1];
    ctrl->acc_count += tail[2];
    int c = ctrl->cursor + 1;
    if (ctrl->wrap > 0 && c >= ctrl->wrap) c = 0;
    ctrl->cursor = c;
    ctrl->iterations = t;
    if constexpr (SCHED) ctrl->lr = lr;  // the rate this step used, for the host to read
  }
}

namespace {

__global__ __launch_bounds__(NT) void sgd_flat_k(float* __restrict__ P, const float* __restrict__ G,
                                                 float* __restrict__ V, uint16_t* __restrict__ Pb, long n, float lr,
                                                 float mom, int nest) {
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
    float wn, vn;
    sgd_update(P[i], G[i], V ? V[i] : 0.f, lr, mom, nest, wn, vn);
    P[i] = wn;
    if (V) V[i] = vn;
    if (Pb) Pb[i] = f2bf(wn);
  }
}

__global__ __launch_bounds__(NT) void sgd_step_k(float* __restrict__ P, const float* __restrict__ G,
                                                 float* __restrict__ V, uint16_t* __restrict__ Pb, long n,
                                                 Ctrl* ctrl, const float* tail) {
  const float lr = ctrl->lr, mom = ctrl->momentum;
  const int nest = ctrl->nesterov;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
    float wn, vn;
    sgd_update(P[i], G[i], mom != 0.f ? V[i] : 0.f, lr, mom, nest, wn, vn);
    P[i] = wn;
    if (mom != 0.f) V[i] = vn;
    Pb[i] = f2bf(wn);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctrl->acc_loss += tail[0];
    ctrl->acc_correct += tail[1];
    ctrl->acc_count += tail[2];
    int c = ctrl->cursor + 1;
    if (ctrl->wrap > 0 && c >= ctrl->wrap) c = 0;
    ctrl->cursor = c;
    ctrl->iterations += 1;
  }
}

// end of an inference step: fold the metric tail into the epoch accumulators (and clear
// it for the next step), advance the cursor
__global__ void step_fold_k(Ctrl* ctrl, float* tail) {
  if (threadIdx.x != 0) return;
  if (tail) {
    ctrl->acc_loss += tail[0];
    ctrl->acc_correct += tail[1];
    ctrl->acc_count += tail[2];
    tail[0] = tail[1] = tail[2] = 0.f;
  }
  int c = ctrl->cursor + 1;
  if (ctrl->wrap > 0 && c >= ctrl->wrap) c = 0;
  ctrl->cursor = c;
}

template <bool REG, int CLIP>
void opt_step_launch(int grid, size_t lds, hipStream_t s, float* P, const float* G, float* S0, float* S1, float* S2,
                     uint16_t* Pb, long n, Ctrl* ctrl, const float* tail, const OptArgs& o, int book,
                     const int32_t* reg, int nreg, long lo, float clipc, const float* scales,
                     const LrSched* sched) {
  if (sched != nullptr)
    hipLaunchKernelGGL((opt_step_k<REG, CLIP, true>), dim3(grid), dim3(NT), lds, s, P, G, S0, S1, S2, Pb, n, ctrl,
                       tail, o, book, reinterpret_cast<const int4*>(reg), nreg, lo, clipc, scales, *sched);
  else
    hipLaunchKernelGGL((opt_step_k<REG, CLIP, false>), dim3(grid), dim3(NT), lds, s, P, G, S0, S1, S2, Pb, n, ctrl,
                       tail, o, book, reinterpret_cast<const int4*>(reg), nreg, lo, clipc, scales, LrSched{});
}

// R = sum over the table's rows of l1 sum|w| + l2 sum(w^2), in a fixed order: block b owns
// the 4-element groups [b per, (b + 1) per) of P (per = ceil(groups / grid), the grid a
// function of n alone); a thread adds its groups (16-byte loads: variables start on
// 8-element boundaries and the padding behind them is zero, so a group lies in one row)
// in fp32, then a wave shuffle tree, one LDS exchange, one partial per block.  The last
// block to arrive adds the partials in block order, re-arms the counter, stores R in
// scratch[grid + 1] and, with a tail, does tail[0] += R * tail[2] (the step's loss sum gains
// R per valid local row).  No float atomics: two launches give the same bits.
// scratch: [grid] partials, [1] arrival counter (int, zero before the first launch), [1] R.
constexpr int RP_MAX_BLOCKS = 1024, RP_U = 4;
__global__ __launch_bounds__(NT) void reg_penalty_k(const float* __restrict__ P, long groups, long per,
                                                    const int4* reg, int nreg, float* scratch, float* tail) {
  extern __shared__ __attribute__((aligned(16))) int4 reg_lds[];
  float* wsum = reinterpret_cast<float*>(reg_lds + nreg);  // [SX_NW], then the election flag
  int* last = reinterpret_cast<int*>(wsum + SX_NW);
  const int b = blockIdx.x, t = threadIdx.x, nb = gridDim.x, lane = t & 63, w = t >> 6;
  reg_stage(reg_lds, reg, nreg);
  RegSeg seg{1, 0, 0.f, 0.f};
  float acc = 0.f;
  const long g1 = (b + 1) * per < groups ? (b + 1) * per : groups;
  // RP_U groups per trip, their loads issued together ahead of the row searches (a small
  // gain: 25.3 us per launch against 26.0 us with one group per trip over ResNet-18's
  // 46.7 MB, back-to-back launches in a captured graph); the groups are still added in
  // ascending order
  for (long g = b * per + t; g < g1; g += RP_U * NT) {
    float4 v[RP_U];
#pragma unroll
    for (int u = 0; u < RP_U; ++u) {
      const long gu = g + u * NT;
      v[u] = gu < g1 ? *reinterpret_cast<const float4*>(P + 4 * gu) : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < RP_U; ++u) {
      const long i = 4 * (g + u * NT);
      if (g + u * NT >= g1) break;
      if (i < seg.off || i >= seg.end) seg = reg_find(reg_lds, nreg, i);
      if (i >= seg.off && i < seg.end) {
        const float s1 = (fabsf(v[u].x) + fabsf(v[u].y)) + (fabsf(v[u].z) + fabsf(v[u].w));
        const float s2 = (v[u].x * v[u].x + v[u].y * v[u].y) + (v[u].z * v[u].z + v[u].w * v[u].w);
        acc += seg.l1 * s1 + seg.l2 * s2;
      }
    }
  }
  acc = sx_wave_sum(acc);
  if (lane == 0) wsum[w] = acc;
  __syncthreads();
  if (t == 0) {
    float v = wsum[0];
#pragma unroll
    for (int u = 1; u < SX_NW; ++u) v += wsum[u];
    scratch[b] = v;
  }
  int* counter = reinterpret_cast<int*>(scratch + nb);
  if (!last_arriver(counter, nb, last)) return;
  float a = 0.f;
  for (int r = t; r < nb; r += NT) a += scratch[r];
  a = sx_wave_sum(a);
  if (lane == 0) wsum[w] = a;
  __syncthreads();
  if (t == 0) {
    float R = wsum[0];
#pragma unroll
    for (int u = 1; u < SX_NW; ++u) R += wsum[u];
    scratch[nb + 1] = R;
    if (tail) tail[0] += R * tail[2];
    *counter = 0;
  }
}

// The L2 norm(s) of the gradient the update rule consumes -- G[i], plus 2 l2 w + l1 sign(w)
// from P for the elements of a regularized variable, the g opt_step_k forms -- and the Keras
// clipping scale(s) c / max(norm, c), in a fixed order.  The layout comes as two tables built
// once by the host: vt, one row (offset, size, l1 bits, l2 bits) per variable, and ct, one
// (start, row of vt) per chunk; every variable is cut into chunks of GN_CHUNK elements, so a
// chunk never spans two variables.  Block b takes chunks b, b + grid, ...: a thread adds the
// squares of its (at most GN_U) 4-element groups, 16-byte loads issued together; a wave
// shuffle tree, one LDS exchange, one partial per CHUNK.  Variables start on 8-element
// boundaries and the padding of G behind them is zero (gather_batch clears G and only
// variables are written; P's padding is zero too), so a chunk's last group may run past the
// variable's end.  The last block to arrive adds each variable's partials in chunk order (16
// lanes per variable: lane j takes chunks j, j + 16, ..., then a shuffle tree) or, for the
// global norm, all of them (reg_penalty_k's order), stores norms and scales and re-arms the
// counter.  No float atomics, a partition that depends on the layout alone: two launches,
// and a graph replay against an eager run, give the same bits.  G (and P) are read once.
// scratch: [nchunk] partials, [1] arrival counter (int, zero before the first launch).
// out: [nout] norms, [nout] scales; nout = nvar (PERVAR) or 1.
constexpr int GN_MAX_BLOCKS = 1024, GN_U = 4;
static_assert(GN_CHUNK == GN_U * NT * 4, "a chunk is one trip of the block");
__device__ __forceinline__ float clip_scale(float norm, float c) {
  // exactly 1.0f while norm <= c (0 included); a non-finite norm poisons the update (NaN)
  const bool finite = (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
  return finite ? c / fmaxf(norm, c) : __uint_as_float(0x7fc00000u);
}
template <bool REG, bool PERVAR>
__global__ __launch_bounds__(NT) void grad_norm_k(const float* __restrict__ G, const float* __restrict__ P,
                                                  const int4* __restrict__ vt, int nvar,
                                                  const int2* __restrict__ ct, int nchunk,
                                                  const int* __restrict__ vfirst, float c, float* scratch,
                                                  float* out) {
  __shared__ float wsums[2][SX_NW];  // two sets, used in turn: one barrier per chunk
  __shared__ int last;
  const int b = blockIdx.x, t = threadIdx.x, nb = gridDim.x, lane = t & 63, w = t >> 6;
  int par = 0;
  for (int ch = b; ch < nchunk; ch += nb, par ^= 1) {
    float* wsum = wsums[par];
    const int2 cd = ct[ch];
    const int4 row = vt[cd.y];
    const int left = row.x + row.y - cd.x;  // elements of the variable from the chunk's start
    const int ngrp = ((left < GN_CHUNK ? left : GN_CHUNK) + 3) >> 2;
    const float l1 = __int_as_float(row.z), l2 = __int_as_float(row.w);
    const bool reg = REG && (l1 != 0.f || l2 != 0.f);  // uniform over the block
    float4 g[GN_U];
#pragma unroll
    for (int u = 0; u < GN_U; ++u) {
      const int gi = t + u * NT;
      g[u] = gi < ngrp ? *reinterpret_cast<const float4*>(G + cd.x + 4 * (long)gi) : float4{0.f, 0.f, 0.f, 0.f};
    }
    if (reg) {
      float4 p[GN_U];
#pragma unroll
      for (int u = 0; u < GN_U; ++u) {
        const int gi = t + u * NT;
        p[u] = gi < ngrp ? *reinterpret_cast<const float4*>(P + cd.x + 4 * (long)gi) : float4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < GN_U; ++u) {  // opt_step_k's expression: the same g, bit for bit
        g[u].x += fmaf(2.f * l2, p[u].x, l1 * (float)((p[u].x > 0.f) - (p[u].x < 0.f)));
        g[u].y += fmaf(2.f * l2, p[u].y, l1 * (float)((p[u].y > 0.f) - (p[u].y < 0.f)));
        g[u].z += fmaf(2.f * l2, p[u].z, l1 * (float)((p[u].z > 0.f) - (p[u].z < 0.f)));
        g[u].w += fmaf(2.f * l2, p[u].w, l1 * (float)((p[u].w > 0.f) - (p[u].w < 0.f)));
      }
    }
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < GN_U; ++u)
      acc += (g[u].x * g[u].x + g[u].y * g[u].y) + (g[u].z * g[u].z + g[u].w * g[u].w);
    acc = sx_wave_sum(acc);
    if (lane == 0) wsum[w] = acc;
    __syncthreads();
    if (t == 0) {
      float v = wsum[0];
#pragma unroll
      for (int u = 1; u < SX_NW; ++u) v += wsum[u];
      scratch[ch] = v;
    }
    // (no second barrier: the next chunk writes the other set, and this set is written
    // again only behind the next chunk's barrier, which thread 0 reaches after this read)
  }
  int* counter = reinterpret_cast<int*>(scratch + nchunk);
  if (!last_arriver(counter, nb, &last)) return;
  if constexpr (PERVAR) {
    // 16 lanes per variable (16 variables at a time: most have one chunk): lane j adds the
    // variable's chunks j, j + 16, ... in order, then a 4-level shuffle tree inside the group
    const int grp = t >> 4, gl = t & 15;
    for (int v0 = 0; v0 < nvar; v0 += NT / 16) {  // the same trip count in every lane
      const int v = v0 + grp;
      float a = 0.f;
      if (v < nvar)
        for (int k = vfirst[v] + gl; k < vfirst[v + 1]; k += 16) a += scratch[k];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o);
      if (v < nvar && gl == 0) {
        const float norm = sqrtf(a);
        out[v] = norm;
        out[nvar + v] = clip_scale(norm, c);
      }
    }
  } else {
    float* wsum = wsums[0];  // (last_arriver's barriers lie behind every read above)
    float a = 0.f;
    for (int k = t; k < nchunk; k += NT) a += scratch[k];
    a = sx_wave_sum(a);
    if (lane == 0) wsum[w] = a;
    __syncthreads();
    if (t == 0) {
      float v = wsum[0];
#pragma unroll
      for (int u = 1; u < SX_NW; ++u) v += wsum[u];
      const float norm = sqrtf(v);
      out[0] = norm;
      out[1] = clip_scale(norm, c);
    }
  }
  if (t == 0) *counter = 0;
}

}  // namespace

hipError_t sgd_flat(float* P, const float* G, float* V, uint16_t* Pb, long n, float lr, float momentum, int nesterov,
                    hipStream_t s) {
  hipLaunchKernelGGL(sgd_flat_k, dim3(grid_for(n, NT, 4096)), dim3(NT), 0, s, P, G, momentum != 0.f ? V : nullptr,
                     Pb, n, lr, momentum, nesterov);
  return hipGetLastError();
}

hipError_t sgd_step(float* P, const float* G, float* V, uint16_t* Pb, long n, Ctrl* ctrl, const float* tail,
                    hipStream_t s) {
  hipLaunchKernelGGL(sgd_step_k, dim3(grid_for(n, NT, 4096)), dim3(NT), 0, s, P, G, V, Pb, n, ctrl, tail);
  return hipGetLastError();
}

hipError_t step_fold(Ctrl* ctrl, float* tail, hipStream_t s) {
  hipLaunchKernelGGL(step_fold_k, dim3(1), dim3(64), 0, s, ctrl, tail);
  return hipGetLastError();
}

hipError_t opt_step(float* P, const float* G, float* S0, float* S1, float* S2, uint16_t* Pb, long n, Ctrl* ctrl,
                    const float* tail, const OptArgs& o, hipStream_t s, int book, const int32_t* reg, int nreg,
                    long lo, int clip, float clipc, const float* scales, const LrSched* sched) {
  if (o.kind < 0 || o.kind > 2 || n < 0) return hipErrorInvalidValue;
  if (sched != nullptr) {
    if (reinterpret_cast<uintptr_t>(sched) & 15) return hipErrorInvalidValue;
    const LrSched& q = *sched;
    if (q.kind < LR_EXPONENTIAL || q.kind > LR_COSINE) return hipErrorInvalidValue;
    if (q.kind == LR_PIECEWISE) {
      if (q.nbounds < 0 || q.nbounds > LR_MAX_BOUNDS) return hipErrorInvalidValue;
      for (int i = 1; i < q.nbounds; ++i)
        if (q.bounds[i] <= q.bounds[i - 1]) return hipErrorInvalidValue;
    } else if (q.decay_steps < 1 || q.decay_steps > LR_MAX_STEPS) {
      return hipErrorInvalidValue;
    }
    if (q.kind == LR_COSINE && (q.flags & 1) && (q.warmup_steps < 0 || q.warmup_steps > LR_MAX_STEPS))
      return hipErrorInvalidValue;
  }
  if (clip < CLIP_NONE || clip > CLIP_GLOBAL) return hipErrorInvalidValue;
  if (clip == CLIP_VALUE && !(clipc > 0.f)) return hipErrorInvalidValue;
  if ((clip == CLIP_VAR || clip == CLIP_GLOBAL) && scales == nullptr) return hipErrorInvalidValue;
  const int grid = n > 0 ? grid_for(n, NT, 4096) : 1;
  const bool table = reg != nullptr && nreg != 0;
  if (clip == CLIP_VAR && !table) return hipErrorInvalidValue;  // the row index comes from the table
  if (table && (nreg < 0 || nreg > REG_MAX_ROWS || lo < 0 || (reinterpret_cast<uintptr_t>(reg) & 15)))
    return hipErrorInvalidValue;
  const size_t lds = table ? nreg * sizeof(int4) : 0;
#define DAMD_OPT_STEP(REG_, CLIP_) \
  opt_step_launch<REG_, CLIP_>(grid, lds, s, P, G, S0, S1, S2, Pb, n, ctrl, tail, o, book, reg, nreg, lo, clipc, \
                               scales, sched)
  if (!table) {
    switch (clip) {
      case CLIP_NONE: DAMD_OPT_STEP(false, CLIP_NONE); break;
      case CLIP_VALUE: DAMD_OPT_STEP(false, CLIP_VALUE); break;
      default: DAMD_OPT_STEP(false, CLIP_GLOBAL); break;
    }
  } else {
    switch (clip) {
      case CLIP_NONE: DAMD_OPT_STEP(true, CLIP_NONE); break;
      case CLIP_VALUE: DAMD_OPT_STEP(true, CLIP_VALUE); break;
      case CLIP_VAR: DAMD_OPT_STEP(true, CLIP_VAR); break;
      default: DAMD_OPT_STEP(true, CLIP_GLOBAL); break;
    }
  }
#undef DAMD_OPT_STEP
  return hipGetLastError();
}

int reg_penalty_blocks(long n) {
  const long groups = n / 4, want = (groups + 4L * NT - 1) / (4L * NT);
  return (int)(want < 1 ? 1 : want > RP_MAX_BLOCKS ? RP_MAX_BLOCKS : want);
}

hipError_t reg_penalty(const float* P, long n, const int32_t* reg, int nreg, float* scratch, float* tail,
                       hipStream_t s) {
  if (n < 0 || n % 4 || nreg < 0 || nreg > REG_MAX_ROWS || scratch == nullptr) return hipErrorInvalidValue;
  if (nreg == 0 || n == 0) return hipSuccess;  // R = 0: nothing to add
  if (reg == nullptr || ((reinterpret_cast<uintptr_t>(reg) | reinterpret_cast<uintptr_t>(P)) & 15))
    return hipErrorInvalidValue;
  const int grid = reg_penalty_blocks(n);
  const long groups = n / 4, per = (groups + grid - 1) / grid;
  const size_t lds = nreg * sizeof(int4) + (SX_NW + 1) * sizeof(float);
  hipLaunchKernelGGL(reg_penalty_k, dim3(grid), dim3(NT), lds, s, P, groups, per, reinterpret_cast<const int4*>(reg),
                     nreg, scratch, tail);
  return hipGetLastError();
}

int grad_norm_blocks(int nchunk) { return nchunk < 1 ? 1 : nchunk > GN_MAX_BLOCKS ? GN_MAX_BLOCKS : nchunk; }

hipError_t grad_norm(const float* G, const float* P, long n, const int32_t* vt, int nvar, const int32_t* ct,
                     int nchunk, const int32_t* vfirst, int per_variable, float c, float* scratch, float* out,
                     hipStream_t s) {
  if (n < 0 || n % 4 || n >= (1L << 31) || nvar < 1 || nchunk < nvar || !(c > 0.f)) return hipErrorInvalidValue;
  if (G == nullptr || vt == nullptr || ct == nullptr || vfirst == nullptr || scratch == nullptr || out == nullptr)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(vt)) & 15)
    return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(ct) & 7) return hipErrorInvalidValue;
  const int grid = grad_norm_blocks(nchunk);
  const int4* v4 = reinterpret_cast<const int4*>(vt);
  const int2* c2 = reinterpret_cast<const int2*>(ct);
#define DAMD_GRAD_NORM(REG_, PV_) \
  hipLaunchKernelGGL((grad_norm_k<REG_, PV_>), dim3(grid), dim3(NT), 0, s, G, P, v4, nvar, c2, nchunk, vfirst, c, \
                     scratch, out)
  if (P != nullptr) {
    if (per_variable) DAMD_GRAD_NORM(true, true); else DAMD_GRAD_NORM(true, false);
  } else {
    if (per_variable) DAMD_GRAD_NORM(false, true); else DAMD_GRAD_NORM(false, false);
  }
#undef DAMD_GRAD_NORM
  return hipGetLastError();
}

}  // namespace damd
