// Non-GEMM per-layer kernels of the generic path, one kernel file per concern under
// csrc/kernels/: bn.hip, pool.hip, loss_head.hip, optimizer.hip, glue.hip, augment.hip.
// Activations are NHWC bf16 (uint16 storage) with the channel count C a multiple of 8,
// parameters / statistics fp32.  All launches are stream-ordered on `s`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace damd {

struct Ctrl;  // kernels_api.h / damd_common.h

// BatchNorm (training) ---------------------------------------------------------------
// Batch statistics without a finalize launch: the producers (conv GEMM epilogue E_STATS
// with GemmArgs::stats_acc, splitk_finish, bn_bwd_reduce / pool_bn_bwd_reduce with `acc`)
// add their per-block fp32 partials into acc[reps][2][C] as int64 fixed point (one word
// per value forward, two backward: damd_common.h bnacc_add1 / bnacc_add2 -- integer
// atomics, so the sums are bitwise independent of the blocks' arrival order); producer
// block / M-tile b adds into replica b % reps, so that same-address atomics --
// serialised at the memory side -- form reps short chains instead of one long one; the
// consumer kernel (bn_apply, bn_relu_maxpool_fwd / bn_bwd_apply, pool_bn_bwd_apply)
// derives the coefficients from acc (replicas summed in order) in its prologue (every
// block, into LDS); its block 0 also writes st / co, the moving statistics and dgamma /
// dbeta.  The accumulators are zeroed once per step (gather_batch's `zero` range).
struct BNFin {
  const long long* acc;  // [reps][2][C] sum, sum of squares (bnacc_add1) + flag plane [2C]; null: the kernel reads st
  const float* gamma;  // may be null (1)
  const float* beta;   // may be null (0)
  float* st;           // [4][C] out (block 0): mean, invstd, scale, shift
  float* rmean;        // moving statistics (block 0), may be null
  float* rvar;
  float count, eps, mom;
  int reps;            // replicas of acc (0 / 1: one)
};
struct BNBwdFin {
  const long long* acc;  // [reps][4][C] sum dz / sum dz * xhat, hi / lo planes (bnacc_add2) + flag plane [4C]; null: co
  float* dgamma;       // += (block 0), may be null
  float* dbeta;
  float* co;           // [3][C] out (block 0)
  float count;
  int reps;
};
// partials [T][2][C] (column sum, sum of squares; from the conv GEMM epilogue) ->
// st[4][C] = mean, invstd, scale = gamma*invstd, shift = beta - mean*scale; moving
// statistics updated Keras-style (m = m*momentum + batch*(1-momentum), biased variance).
hipError_t bn_finalize(const float* part, int T, int C, float count, const float* gamma, const float* beta,
                       float eps, float momentum, float* rmean, float* rvar, float* st, hipStream_t s);
// y = act(x*scale + shift [+ r | + r*scale2 + shift2])   (res_mode 0 / 1 / 2)
hipError_t bn_apply(const uint16_t* x, const float* st, const uint16_t* r, const float* st2, int res_mode,
                    int relu, uint16_t* y, long M, int C, hipStream_t s, const BNFin* f1 = nullptr,
                    const BNFin* f2 = nullptr);
// backward, pass 1: dz = dy * [y > 0] (relu_mask 1; relu_mask 2: y recomputed as
// bf16(relu(x * sc + sh)) from x and st, bitwise the stored bn_apply output, y unread);
// per-block partial sums of dz and dz * xhat -> part [T][2][C] (T blocks), or into acc;
// optionally writes dz (bf16)
hipError_t bn_bwd_reduce(const uint16_t* dy, const uint16_t* y, int relu_mask, const uint16_t* x,
                         const float* st, uint16_t* dz_out, float* part, int T, long M, int C, hipStream_t s,
                         long long* acc = nullptr, int acc_reps = 1);
int bn_bwd_blocks(long M, int C);
// tests: bn_bwd_reduce launches its row ranges in reversed block order (order independence)
void bn_reduce_reverse(bool on);
// pass 2: dgamma/dbeta (accumulated into the gradient sinks, may be null) and the
// coefficients co[3][C] so that dx = a*dz + b + c*xhat
hipError_t bn_bwd_finalize(const float* part, int T, int C, float count, const float* st, float* dgamma,
                           float* dbeta, float* co, hipStream_t s);
// pass 3: dx = a*dz + b + c*xhat, dz recomputed from dy and the relu mask (bf16 out)
hipError_t bn_bwd_apply(const uint16_t* dy, const uint16_t* y, int relu_mask, const uint16_t* x, const float* st,
                        const float* co, uint16_t* dx, long M, int C, hipStream_t s, const BNBwdFin* bf = nullptr);

// Two BatchNorms of the same masked gradient (relu_mask 0 / 1), fixed-point accumulators
// and in-consumer finalize only: one reduce pass and one apply pass for both (bitwise the
// two single-BN launch pairs)
hipError_t bn_bwd_reduce_dual(const uint16_t* dy, const uint16_t* y, int relu_mask, const uint16_t* x,
                              const uint16_t* x2, const float* st, const float* st2, int T, long M, int C,
                              hipStream_t s, long long* acc, long long* acc2, int acc_reps);
hipError_t bn_bwd_apply_dual(const uint16_t* dy, const uint16_t* y, int relu_mask, const uint16_t* x,
                             const uint16_t* x2, const float* st, const float* st2, uint16_t* dx, uint16_t* dx2,
                             long M, int C, hipStream_t s, const BNBwdFin& bf, const BNBwdFin& bf2);

// Pooling ----------------------------------------------------------------------------------
// x [N][H][W][C], windows ph x pw, strides sh x sw, pt / pl rows / columns of padding above /
// left of the input, y [N][Ho][Wo][C].  The field order is that of ops/hip.py pool_geo(),
// whose 12-int list the bindings turn into this struct; the kernels take it by value.
struct PoolGeo {
  int N, H, W, C, ph, pw, sh, sw, pt, pl, Ho, Wo;
};
hipError_t maxpool_fwd(const uint16_t* x, const PoolGeo& g, uint16_t* y, uint8_t* arg, hipStream_t s);
hipError_t maxpool_bwd(const uint16_t* dy, const uint8_t* arg, const PoolGeo& g, uint16_t* dx, hipStream_t s);
// average pooling, divisor = in-bounds taps (TF 'same' semantics)
hipError_t avgpool_fwd(const uint16_t* x, const PoolGeo& g, uint16_t* y, hipStream_t s);
hipError_t avgpool_bwd(const uint16_t* dy, const PoolGeo& g, uint16_t* dx, hipStream_t s);
// stem fusion (BatchNorm(st) -> ReLU -> MaxPool): the pool reads the conv output x
hipError_t bn_relu_maxpool_fwd(const uint16_t* x, const float* st, const PoolGeo& g, uint16_t* y, uint8_t* arg,
                               hipStream_t s, const BNFin* f = nullptr);
// its backward: BN-backward partials / apply with the pool routing + ReLU mask recomputed
hipError_t pool_bn_bwd_reduce(const uint16_t* dpool, const uint8_t* arg, const PoolGeo& g, const uint16_t* x,
                              const float* st, float* part, int T, hipStream_t s, long long* acc = nullptr,
                              int acc_reps = 1);
hipError_t pool_bn_bwd_apply(const uint16_t* dpool, const uint8_t* arg, const PoolGeo& g, const uint16_t* x,
                             const float* st, const float* co, uint16_t* dx, hipStream_t s,
                             const BNBwdFin* bf = nullptr);
// global average pool over H*W: x [N][HW][C] bf16 -> y [N][C] (bf16 or fp32)
hipError_t gap_fwd(const uint16_t* x, int N, int HW, int C, void* y, int y_f32, hipStream_t s);
hipError_t gap_bwd(const void* dy, int dy_f32, int N, int HW, int C, uint16_t* dx, hipStream_t s);

// Depthwise convolution (csrc/kernels/dwconv.hip), depth_multiplier 1 ------------------------
// PoolGeo with ph x pw the kernel; w: the taps [ph * pw][C] bf16 (16-byte aligned).
// y = bf16(act(sum of the in-bounds taps (fp32, (i, j) order) + bias)); bias fp32 [C] or null,
// relu 0 / 1
hipError_t dwconv_fwd(const uint16_t* x, const uint16_t* w, const float* bias, int relu, const PoolGeo& g,
                      uint16_t* y, hipStream_t s);
// dx = the gather of dy over the taps that reach each input pixel; EVERY dx element is written
hipError_t dwconv_dgrad(const uint16_t* dy, const uint16_t* w, const PoolGeo& g, uint16_t* dx, hipStream_t s);
// dw [ph * pw][C] fp32 += sum over the output pixels of x * dy, in a fixed order (no float
// atomics): dwconv_wgrad_blocks(g) pixel slabs write one partial row each into ws
// ([blocks][ph * pw * C] fp32), a second pass adds the rows in order.  Square kernels up to 7 x 7.
int dwconv_wgrad_blocks(const PoolGeo& g);
hipError_t dwconv_wgrad(const uint16_t* x, const uint16_t* dy, const PoolGeo& g, float* dw, float* ws, hipStream_t s);
// blocks a forward / backprop-input launch runs at most (grid-stride beyond)
int dwconv_grid_cap();

// Elementwise -----------------------------------------------------------------------------
// dz = dy * [y > 0]  (bf16)
hipError_t relu_bwd(const uint16_t* dy, const uint16_t* y, uint16_t* dz, long n, hipStream_t s);
// y = act(x) / dx = dy * act'(y), kind 0 relu, 1 sigmoid, 2 tanh (bf16, any length, in place ok)
hipError_t act_fwd(const uint16_t* x, uint16_t* y, long n, int kind, hipStream_t s);
hipError_t act_bwd(const uint16_t* dy, const uint16_t* y, uint16_t* dx, long n, int kind, hipStream_t s);
// y = x * keep / (1 - rate), keep from a counter hash of (seed, ctrl->cur3, element): the
// same call with the same seed is the backward (dx from dy)
hipError_t dropout(const uint16_t* x, uint16_t* y, long n, const Ctrl* ctrl, uint32_t seed, float rate,
                   hipStream_t s);
// Inference: BN st rows from the moving statistics; this step's logits rows -> out at the
// device cursor; fold the metric tail into ctrl (tail cleared) and advance the cursor
hipError_t bn_infer_st(const float* rmean, const float* rvar, const float* gamma, const float* beta, float eps, int C,
                       float* st, hipStream_t s);
hipError_t logits_store(const float* logits, int ld, int K, int B, const Ctrl* ctrl, float* out, hipStream_t s);
// logits_store with a row softmax (models whose output is a probability); both reject
// K < 1, K > ld, B < 1 and a null ctrl before any launch
hipError_t softmax_store(const float* logits, int ld, int K, int B, const Ctrl* ctrl, float* out, hipStream_t s);
hipError_t step_fold(Ctrl* ctrl, float* tail, hipStream_t s);
// out = a + b (bf16)
hipError_t add_bf16(const uint16_t* a, const uint16_t* b, uint16_t* out, long n, hipStream_t s);
// fp32 -> bf16, bf16 -> fp32
hipError_t cast_f32_bf16(const float* x, uint16_t* y, long n, hipStream_t s);
hipError_t cast_bf16_f32(const uint16_t* x, float* y, long n, hipStream_t s);
// uint8 (k) -> bf16(k * scale)
hipError_t cast_u8_bf16(const uint8_t* x, float scale, uint16_t* y, long n, hipStream_t s);
// out[n] += sum_m x[m][n]  (x bf16 or fp32, [M][ld]) in a fixed order; when
// colsum_splits(M, N) > 1 the row splits go through ws[splits][N] (fp32 workspace)
int colsum_splits(int M, int N);
hipError_t colsum(const void* x, int x_f32, int M, int N, int ld, float* out, float* ws, hipStream_t s);

// Loss --------------------------------------------------------------------------------------
// Sparse softmax cross-entropy from fp32 logits [B][ld]: dlogits (bf16, [B][K]) =
// (softmax - onehot) * scale; tail[0] += sum loss, tail[1] += sum correct (argmax ==
// label, first max wins), tail[2] += B.  labels int32; a label < 0 masks the row (zero
// gradient, no loss/metric).  ctrl != nullptr: scale = 1 / real rows of the global batch
// (short final batch; see softmax_xent_k), else the given scale.
// dlogits shares the row pitch ld of the logits; its padding columns are left untouched.
// rows: scratch of 3 B floats + one int arrival counter (zero before the first call; the
// kernel re-arms it): the batch sums are formed in a fixed order, not by float atomics.
// bias_grad (optional): += the column sums of the stored dlogits, exactly as colsum with one
// split (the logits layer's bias gradient without a colsum launch)
// weights (optional, fp32): row b's gradient and loss are multiplied by its weight, the correct
// and valid counts are not.  ctrl == nullptr: weights[b]; else the weight of the sample at the
// device cursor, weights[cursor * global_batch + row0 + b] (modulo nsamples in wrap mode).  A
// row with label < 0 does not read the array.  nullptr launches the unweighted kernel.
hipError_t softmax_xent(const float* logits, int ld, const int32_t* labels, int B, int K, float scale,
                        const Ctrl* ctrl, uint16_t* dlogits, float* tail, float* rows, hipStream_t s,
                        float* bias_grad = nullptr, const float* weights = nullptr);
// The same against dense fp32 target rows [.][K] (one-hot or soft; label_smoothing eps in
// [0, 1): y' = y (1 - eps) + eps / K): loss = -sum y' log softmax, dlogits = (softmax *
// sum y' - y') * scale, correct = argmax logits == argmax y (first max wins on both).
// ctrl != nullptr: block b reads target row cursor * global_batch + row0 + b (modulo
// nsamples in wrap mode) of the epoch-ordered targets and labels[b] < 0 masks the row;
// ctrl == nullptr: target row b, labels optional.  tail / rows / bias_grad as softmax_xent;
// weights are indexed by the target row.
hipError_t softmax_xent_dense(const float* logits, int ld, const int32_t* labels, const float* targets, int B, int K,
                              float label_smoothing, float scale, const Ctrl* ctrl, uint16_t* dlogits, float* tail,
                              float* rows, hipStream_t s, float* bias_grad = nullptr,
                              const float* weights = nullptr);

// Optimizer ---------------------------------------------------------------------------------
// flat multi-tensor Keras SGD over the master buffer: P, V fp32 updated from G; Pb = bf16(P)
hipError_t sgd_flat(float* P, const float* G, float* V, uint16_t* Pb, long n, float lr, float momentum,
                    int nesterov, hipStream_t s);

// one training step's optimizer tail for the graph-captured generic path: hyper-parameters
// from ctrl (lr / momentum / nesterov, so a new lr needs no re-capture); block 0 also
// folds the step's metric tail [loss, correct, count] into the epoch accumulators and
// advances ctrl->cursor / ctrl->iterations.
hipError_t sgd_step(float* P, const float* G, float* V, uint16_t* Pb, long n, Ctrl* ctrl, const float* tail,
                    hipStream_t s);
// kind 0 SGD (S0 momentum; flag = nesterov), 1 Adam (S0 m, S1 v, S2 vhat; flag = amsgrad),
// 2 RMSprop (S0 rms, S1 momentum, S2 mean gradient; flag = centered)
struct OptArgs {
  int kind;
  float b1, b2, eps, rho, mom;
  int flag;
};
// reg (optional): the weight-regularizer segment table, nreg rows of 4 words (offset, size,
// l1 as float bits, l2 as float bits) sorted by offset, 16-byte aligned, nreg <= REG_MAX_ROWS;
// offsets are absolute in the engine's flat buffer and P[0] is its element `lo`.  Each
// element of a row uses g + 2 l2 w + l1 sign(w) as its gradient.  reg == nullptr or
// nreg == 0: the kernel without any regularizer code.
//
// clip: Keras gradient clipping of that (regularized) gradient before the update rule.
// 0 none; 1 value: clamp to [-clipc, clipc]; 3 global: g * scales[0]; 2 per variable:
// g * scales[row], where the table must then list EVERY variable (zero coefficients where
// there is no regularizer; nreg = the number of variables <= REG_MAX_ROWS) and row is the
// element's row -- the index grad_norm stores its scales under.  scales: grad_norm's output.
// clip == 0 is the kernel without any clipping code.
//
// sched (optional): a Keras learning-rate schedule (keras/schedules.py) evaluated on the
// device.  Every thread computes lr = f(ctrl->cur3 - 1) -- the optimizer's iterations before
// this update -- once before its element loop, in fp32, with all step logic (staircase
// floor, cycle ceil, clamps, boundary search, warm-up branch) in integer arithmetic; the
// update rules (Adam's lr_t included) use it instead of ctrl->lr, and the bookkeeping launch
// stores it into ctrl->lr for the host to read (under a schedule no launch reads that
// field).  The descriptor is LR_WORDS 32-bit words in HOST memory, 16-byte aligned (build it
// with ops/hip.py lr_table); opt_step checks it and hands it to the kernel by value, as a
// kernel argument: the words arrive in scalar registers with the other arguments -- no
// table load, provably wave-uniform -- and are a constant of a captured step, like clipc.
// sched == nullptr is the kernel without any schedule code, reading ctrl->lr.
constexpr int LR_MAX_BOUNDS = 16;  // boundaries of a PiecewiseConstantDecay
constexpr int LR_MAX_STEPS = 1 << 24;  // decay_steps / warmup_steps: exact as a float
enum : int { LR_EXPONENTIAL = 1, LR_INVERSE_TIME = 2, LR_POLYNOMIAL = 3, LR_PIECEWISE = 4, LR_COSINE = 5 };
struct alignas(16) LrSched {
  int32_t kind;          // 0  LR_*
  int32_t flags;         // 1  bit 0: staircase (1, 2) / cycle (3) / warm-up (5)
  int32_t decay_steps;   // 2  in [1, LR_MAX_STEPS] (kind 4: unused)
  int32_t warmup_steps;  // 3  in [0, LR_MAX_STEPS] (kind 5 with warm-up)
  float init;            // 4  initial_learning_rate
  float a;               // 5  decay_rate (1, 2) / end_learning_rate (3) / alpha (5)
  float b;               // 6  power (3) / warmup_target (5)
  int32_t nbounds;       // 7  kind 4: boundaries in use, <= LR_MAX_BOUNDS
  int32_t bounds[LR_MAX_BOUNDS];     // 8   strictly increasing
  float values[LR_MAX_BOUNDS + 1];   // 24  nbounds + 1 in use
  int32_t pad[3];
};
constexpr int LR_WORDS = sizeof(LrSched) / 4;
static_assert(sizeof(LrSched) == 44 * 4, "ops/hip.py lr_table lays these words out");
constexpr int REG_MAX_ROWS = 2048;  // 32 KB of LDS per block
hipError_t opt_step(float* P, const float* G, float* S0, float* S1, float* S2, uint16_t* Pb, long n, Ctrl* ctrl,
                    const float* tail, const OptArgs& o, hipStream_t s, int book = 1, const int32_t* reg = nullptr,
                    int nreg = 0, long lo = 0, int clip = 0, float clipc = 0.f, const float* scales = nullptr,
                    const LrSched* sched = nullptr);
// The L2 norm of the gradient opt_step consumes -- G, plus 2 l2 w + l1 sign(w) from the
// masters P where vt has coefficients (P == nullptr: G alone, P is not read) -- per variable
// (per_variable != 0) or over all variables, and the clipping scale c / max(norm, c): exactly
// 1.0f up to norm == c (a zero gradient included), NaN for a non-finite norm.  One launch,
// fixed summation order, no float atomics: repeated launches give the same bits.
// G / P: n floats (n a multiple of 4 below 2^31, 16-byte aligned); variables start on
// 8-element boundaries and the padding behind them is ZERO in both buffers -- the kernel
// reads whole 4-element groups and relies on it, as reg_penalty relies on P's padding.
// vt: nvar rows (offset, size, l1 bits, l2 bits) sorted by offset, 16-byte aligned, one per
// variable.  ct: nchunk rows (start, row of vt): every variable cut into chunks of GN_CHUNK
// elements in ascending order, no chunk spanning two variables.  vfirst: nvar + 1 words, the
// first chunk of each variable (vfirst[nvar] = nchunk).  scratch: nchunk + 1 words, zero
// before the first launch (per-chunk partials, the arrival counter the launch re-arms).
// out: 2 * nout floats, the norms then the scales; nout = nvar (per variable) or 1.
// The tables live on the device and are trusted: build them with ops/hip.py clip_plan.
constexpr int GN_CHUNK = 4096;
int grad_norm_blocks(int nchunk);
hipError_t grad_norm(const float* G, const float* P, long n, const int32_t* vt, int nvar, const int32_t* ct,
                     int nchunk, const int32_t* vfirst, int per_variable, float c, float* scratch, float* out,
                     hipStream_t s);
// R = sum over the table's rows of l1 sum|w| + l2 sum(w^2) over the flat fp32 buffer P[n]
// (n a multiple of 4, P 16-byte aligned, rows starting on 8-element boundaries with zero
// padding behind them), summed in a fixed order (no float atomics).  scratch holds
// reg_penalty_blocks(n) + 2 words, zero before the first launch: per-block partials, the
// arrival counter (re-armed by the launch) and R, which the host may read.  tail (optional):
// tail[0] += R * tail[2] -- the loss sum of a step gains R for each of its valid rows.
// nreg == 0 launches nothing.
int reg_penalty_blocks(long n);
hipError_t reg_penalty(const float* P, long n, const int32_t* reg, int nreg, float* scratch, float* tail,
                       hipStream_t s);

// Data / layout glue -------------------------------------------------------------------------
// the step's rows of the (epoch-permuted) dataset: row = (cursor*global_batch + row0 + i)
// mod nsamples (cursor from ctrl); x fp32 or uint8 (k / scale, i.e. exactly float32(k/255)
// for scale 255) [n][HW][Cin] -> bf16
// [per][HW][Cp] zero-padded channels; labels int32.  zero / zero2 (optional): byte ranges
// (16-byte aligned, multiples of 16 bytes) cleared in the same launch -- the step's
// gradient buffer and BatchNorm statistics accumulators, so no memset launch precedes it.
// uint8 RGB into Cp == 4 with HW % 4 == 0 reads x as dwords: x must be 4-byte aligned.
// A pad_cast (below) run inside gather_batch's launch: the step's first layer's padded bf16
// weights refreshed without a launch of their own (src == nullptr: none).
struct PadCastJob {
  const float* src;
  uint16_t* dst;
  int R, C1, C2, C1p, C2p;
};
hipError_t gather_batch(const void* x, int x_u8, float scale, const int32_t* labels, Ctrl* ctrl, int per,
                        int HW, int Cin, int Cp, uint16_t* xb, int32_t* yb, hipStream_t s, void* zero = nullptr,
                        long zero_bytes = 0, void* zero2 = nullptr, long zero2_bytes = 0,
                        PadCastJob pc = PadCastJob{nullptr, nullptr, 0, 0, 0, 0, 0});
// Input augmentation (csrc/kernels/augment.hip): the model's input prefix -- a chain of
// ZeroPadding2D / RandomCrop / RandomFlip layers -- as ONE launch behind gather_batch.
// x [B][H][W][Cp] bf16 -> y [B][Ho][Wo][Cp]: every output pixel is a whole input pixel or
// zero (no arithmetic on values).  The stages are listed in layer order; a thread maps its
// output pixel back through them from the last to the first:
//   AUG_FLIP  p = {mode bits (1 left-right, 2 up-down)}: mirrors the drawn axes
//   AUG_CROP  p = {out_h, out_w}: adds the drawn offset in [0, in - out]
//   AUG_PAD   p = {top, bottom, left, right}: subtracts (top, left); a coordinate outside
//             the stage's input is a pad band and the pixel is zero (whatever the earlier
//             stages are)
// (a stage's input size follows from H x W and the stages ahead of it.)
// The draws of sample b are a pure function of (stage seed, t = ctrl->cur3, g = ctrl->row0 + b)
// -- neither rank nor world size enter -- computed once per block (blockIdx.y = b) from
// scalars: h = mix32(mix32(g ^ key) + key), key = mix32(seed + t * 0x9e3779b9); flips are
// bits 31 (left-right) and 30 (up-down) of h, crop offsets h % (in_h - out_h + 1) and
// mix32(h + key) % (in_w - out_w + 1).  training == 0: no flip, centred crops.
// labels[b] < 0 (a row past the end of the data, as gather_batch marks it): zeros.
// ops/hip.py augment_reference is the host oracle.  The table is AUG_WORDS 32-bit words in
// HOST memory (ops/hip.py aug_table); augment checks it against the shapes (the chain leads
// from H x W to Ho x Wo, no crop larger than its input) and hands
// it to the kernel by value, like opt_step's LrSched: a constant of a captured step.
constexpr int AUG_MAX_STAGES = 8;
enum : int { AUG_FLIP = 1, AUG_CROP = 2, AUG_PAD = 3 };
struct AugStage {
  int32_t kind;
  int32_t p[4];
  uint32_t seed;
  int32_t pad[2];
};
struct alignas(16) AugTable {
  int32_t n;  // stages in use, 1 .. AUG_MAX_STAGES
  int32_t pad[3];
  AugStage st[AUG_MAX_STAGES];
};
constexpr int AUG_WORDS = sizeof(AugTable) / 4;
static_assert(sizeof(AugTable) == 68 * 4, "ops/hip.py aug_table lays these words out");
hipError_t augment(const uint16_t* x, uint16_t* y, const int32_t* labels, const Ctrl* ctrl, const AugTable* tab, int B,
                   int H, int W, int Ho, int Wo, int Cp, int training, hipStream_t s);

// fp32 [R][C1][C2] -> bf16 [R][C1p][C2p] (zero padding)
hipError_t pad_cast(const float* src, int R, int C1, int C2, int C1p, int C2p, uint16_t* dst, hipStream_t s);
// dst fp32 [R][C1][C2] += src fp32 [R][C1p][C2p] (the un-padded part)
hipError_t unpad_add(const float* src, int R, int C1, int C2, int C1p, int C2p, float* dst, hipStream_t s);

}  // namespace damd
