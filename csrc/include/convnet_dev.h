// Device-side building blocks of the fused MNIST-CNN step kernels
// (csrc/kernels/convnet_step2.hip): model constants and flat-buffer layout, input-row
// staging, the conv 3x3 + bias + ReLU + 2x2 max-pool on MFMA, fixed-point sums.
#pragma once
#include "convnet.h"
#include "damd_common.h"

namespace damd {
namespace convnet {

constexpr int IMG = 28, NPIX = IMG * IMG;
constexpr int PO = 13, NPOS = PO * PO;      // pooled 13x13
constexpr int NF = 32;                       // conv filters
constexpr int FEAT = NPOS * NF;              // 5408
constexpr int HID = 64, NCLS = 10;
constexpr int OFF_WC = 0, OFF_BC = 288, NCONV = 320;
constexpr int OFF_W1 = NCONV, OFF_B1 = OFF_W1 + FEAT * HID;
constexpr int OFF_W2 = OFF_B1 + HID, OFF_B2 = OFF_W2 + HID * NCLS;
constexpr int NPARAM = OFF_B2 + NCLS;        // 347146
constexpr int OFF_LOSS = NPARAM, OFF_CORR = NPARAM + 1, OFF_CNT = NPARAM + 2;
constexpr int NGRAD = NPARAM + 6;            // padded to 16 B: 347152
constexpr int NSMALL = HID + HID * NCLS + NCLS;  // b1, W2, b2 contiguous: 714
constexpr int CH = 64;                       // images per chunk
constexpr int LG_CH = 6;                     // log2(CH)
// dense-1 accumulator row pitch (int64 elements): one 512-B row of 64 sums per image.
// Contiguous (64) is the default: rows 4 KB apart, to spread the forward's 57-deep
// same-address atomic chains over more memory channels, measured +1.1 us per step (the
// backward started 0.95 us later; same-box A/B, round 5)
#ifndef DAMD_HACC_PITCH
#define DAMD_HACC_PITCH 64
#endif
constexpr int HACC_PITCH = DAMD_HACC_PITCH;
constexpr int XR = 6;                        // staged input rows per image
constexpr int MAXPP = 4;                     // max pooled positions per fwd / bwd block
constexpr int XS_BYTES = CH * XR * IMG * 4;  // 43008
constexpr int HP = 72;                       // bf16 pitch of 64-wide tiles (conflict-free)
static_assert(CH == 1 << LG_CH, "chunk size");
static_assert(HACC_PITCH >= 64 && HACC_PITCH % 64 == 0, "hacc pitch");
static_assert(NPARAM == kConvNetNParam && NGRAD == kConvNetNGrad, "param count");

__host__ __device__ constexpr int kpitch(int pp) { return pp * 32 + 8; }
__host__ __device__ constexpr int nsp(int ns) { return (ns + 3) & ~3; }

__device__ __forceinline__ uint16_t bf16_lo(float v, uint16_t hi) { return f2bf(v - bf2f(hi)); }

// next step index (wraps for benchmark epochs)
__device__ __forceinline__ int next_cursor(const Ctrl& c, int cur) {
  return (c.wrap > 0 && cur + 1 >= c.wrap) ? 0 : cur + 1;
}

// ---- staged input rows: registers first (loads in flight early), LDS later ------------
// A block stages rows [r0, r0 + nrows) of nimg = 2^lgi images (16 or 64) into the
// [nimg][XR][28] LDS tile.  One unit = 4 pixels: 4 B (u8) or 16 B (fp32).  Thread t owns
// column unit q = t & 7 (q = 7: idle) of rows rg, rg + RG, ... of image t >> (9 - lgi),
// where 512 / nimg threads share an image in RG = 2^(6 - lgi) row groups (64 images: all 6
// rows per thread; 16: rows rg, rg + 4).  Shifts only: the former linear unit index took a
// division per unit -- ~20 VALU each, quarter-rate multiplies among them -- and the
// prologue of both step kernels is VALU-issue bound (two waves per SIMD, wave64 over 16
// lanes: 4 clocks per VALU instruction).
template <bool U8>
struct XStage;
template <>
struct XStage<true> {
  uint32_t w[XR];
  int off, rg;  // LDS float offset of (image, row rg, unit q), -1: idle lane; row group
};
template <>
struct XStage<false> {
  float4 v[XR];
  int off, rg;
};
// Images b < nvalid with row_base + b < nsamples are loaded, others staged as zeros.
// U8: the dataset is kept as uint8 (inputs that are exactly k/255, e.g. MNIST) -- 4x fewer
// bytes -- and k/255.f (correctly rounded, == float32(k/255.0)) is formed when staging;
// otherwise fp32 rows.  32-bit sample indices and byte offsets (the engine keeps the
// dataset below 2^31 bytes), so the loads take the scalar-base + 32-bit-offset form.
// t: the staging slot (thread index by default; a block may give one thread two slots)
template <bool U8>
__device__ __forceinline__ void x_load(XStage<U8>& st, const void* __restrict__ X, long row_base, int nsamples,
                                       int nvalid, int lgi, int r0, int nrows, int t = (int)threadIdx.x) {
  const int sh = 9 - lgi, b = t >> sh, rg = (t & ((1 << sh) - 1)) >> 3, q = t & 7;
  const int RG = 1 << (6 - lgi);
  const int g = (int)row_base + b;
  const bool ok = b < nvalid && g < nsamples && q < 7;
  st.off = q < 7 ? (b * XR + rg) * IMG + 4 * q : -1;
  st.rg = rg;
  // element offset of (row r0 + rg, unit q); rows advance by RG * IMG elements
  const unsigned eo = __umul24((unsigned)max(0, min(g, nsamples - 1)), (unsigned)NPIX) + (unsigned)((r0 + rg) * IMG + 4 * q);
  // one 64-bit base per thread, rows at a uniform byte stride (per-row 32-bit offsets became
  // a quarter-rate 64-bit multiply-add per row)
  constexpr int ES = U8 ? 1 : 4;
  const char* xb = static_cast<const char*>(X) + (size_t)eo * ES;
  const int rstride = RG * IMG * ES;
#pragma unroll
  for (int j = 0; j < XR; ++j) {
    if constexpr (U8) st.w[j] = 0u;
    else st.v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j * RG >= XR) continue;  // (uniform)
    if (ok && rg + j * RG < nrows) {
      const char* pj = xb + j * rstride;
      if constexpr (U8) st.w[j] = *reinterpret_cast<const uint32_t*>(pj);
      else st.v[j] = *reinterpret_cast<const float4*>(pj);
    }
  }
}

// k / 255 rounded to fp32 exactly as float32(k / 255.0) for every k < 256 (checked for all
// 256 with exact fma arithmetic): q = k * (1/255) plus one fma-residual correction -- three
// VALU ops instead of a correctly rounded division (~10) or an LDS table read (a serial
// LDS round trip per staged unit)
__device__ __forceinline__ float u8_over_255(uint32_t k) {
  const float r = 1.f / 255.f, x = (float)k, q = x * r;
  return fmaf(fmaf(-q, 255.f, x), r, q);
}
template <bool U8>
__device__ __forceinline__ void x_store(const XStage<U8>& st, float* xs, int lgi, int nrows) {
  const int RG = 1 << (6 - lgi);
  if (st.off < 0) return;
#pragma unroll
  for (int j = 0; j < XR; ++j) {
    if (j * RG >= XR) continue;  // (uniform)
    if (st.rg + j * RG < nrows) {
      float4 v;
      if constexpr (U8) {
        const uint32_t w = st.w[j];
        v = make_float4(u8_over_255(w & 0xff), u8_over_255((w >> 8) & 0xff), u8_over_255((w >> 16) & 0xff),
                        u8_over_255(w >> 24));
      } else {
        v = st.v[j];
      }
      *reinterpret_cast<float4*>(xs + st.off + j * RG * IMG) = v;
    }
  }
}

// ---- conv 3x3 + bias + ReLU + 2x2 max-pool of a slice on MFMA ----
// One 16x16x32 bf16 MFMA per tile with a split-precision K packing:
//   k in [0,9): x_hi*w_hi   [9,18): x_lo*w_hi   [18,27): x_hi*w_lo   [27,32): 0
// (x = hi + lo, w = hi + lo in bf16) -> ~16-bit-mantissa conv outputs, so the pool
// argmax / ReLU mask match an fp32 conv; the 23 spare K slots of a 9-tap conv pay it.
// Row tile rt = 4 pool windows x 4 sub-pixels (window wi = pl*64 + image), so the 4
// pixels of one window are the 4 accumulator rows of one lane: bias + ReLU + max +
// first-max argmax happen in registers.
//
// The conv phase is VALU-issue bound and at 12 waves each wave builds exactly one tile, so
// whatever depends only on the lane, the wave or the slice is kept out of its stream:
//   * the weight fragments lie in LDS in operand order (wf, conv_w_store): the thread that
//     updates a weight splits it and stores the halves into the K slots that take them;
//     conv_setup is two 16-byte reads and two bias reads per lane;
//   * K slot 8 kg + j of lane group kg = lane >> 4 holds tap (j - kg) mod 9, so the 8 gather
//     offsets and the hi / lo / zero choice of every slot depend on kg only: they are
//     constants picked by kg (one byte per offset, one byte-permute selector per slot pair);
//   * the tile's coordinates are wave-uniform (callers pass a readfirstlane'd wave, and the
//     4 windows of a tile share wi >> lg for lg >= 2): position, division by 13 and row base
//     are scalar work, the lane adds a constant of its own.
constexpr int WF_BYTES = 2 * 64 * 16;            // wf[nt][lane]: one bf16x8 B fragment each
constexpr int CONV_LDS_BYTES = WF_BYTES + NF * 4;  // + [32] fp32 biases
struct ConvFrag {
  bf16x8 w[2];
  float bias[2];
  int lbase;        // byte offset in xs of the lane's pixel (window r >> 2, sub-pixel r & 3) within the tile
  uint32_t tb[2];   // byte offsets of the 8 gathers, one per byte
  uint32_t sel[4];  // v_perm selectors of the 4 slot pairs: hi, lo or zero per half
};
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
// byte offset of tap t = (ty, tx) from a window pixel
constexpr uint32_t tap_off4(int t) { return 4u * (uint32_t)(t + (IMG - 3) * (t / 3)); }
constexpr uint32_t gather_word(int kg, int half) {
  uint32_t w = 0;
  for (int i = 0; i < 4; ++i) w |= tap_off4((4 * half + i - kg + 9) % 9) << (8 * i);
  return w;
}
// v_perm_b32(hi pair, lo pair, sel): selector bytes 4-7 take the hi pair's bytes, 0-3 the lo
// pair's, 0x0c gives 0x00.  K slot k takes x_hi (k < 9 and 18 <= k < 27), x_lo (9 <= k < 18)
// or zero (k >= 27); element e of a pair fills the low (e = 0) or high half of the word.
constexpr uint32_t half_sel(int k, int e) {
  return k >= 27 ? 0x0c0cu : (k >= 9 && k < 18) ? (e ? 0x0302u : 0x0100u) : (e ? 0x0706u : 0x0504u);
}
constexpr uint32_t pair_sel(int kg, int p) {
  return half_sel(8 * kg + 2 * p, 0) | (half_sel(8 * kg + 2 * p + 1, 1) << 16);
}
static_assert(tap_off4(8) < 256, "gather offsets fit a byte");
// index (bf16 elements) in wf of K slot k of channel c: fragment nt = c >> 4, lane
// (k >> 3) * 16 + (c & 15), element k & 7
__device__ __forceinline__ int wf_slot(int k, int c) {
  return (((c >> 4) * 64 + (c & 15)) << 3) + ((k >> 3) << 7) + (k & 7);
}
// The thread that owns the update of conv weight (tap t, channel c) splits it once
// (w = hi + lo in bf16) and stores the halves where the MFMA operand takes them: hi at K
// slots t and t + 9, lo at t + 18 (split per wave and lane, the conversions, selects and
// packing sat on the conv phase's VALU-issue-bound path once per wave).
// ws: the thread's slots (conv_w_slots), computed ahead of the loads the update waits for.
__device__ __forceinline__ void conv_w_store(uint16_t* wf, const int* ws, float w32) {
  const uint16_t hi = f2bf(w32), lo = bf16_lo(w32, hi);
  wf[ws[0]] = hi;
  wf[ws[1]] = hi;
  wf[ws[2]] = lo;
}
// Thread i < 288 owns conv weight i = (tap i >> 5, channel i & 31): its three slots.  Threads
// NCONV <= i < NCONV + 160 zero the 5 x 32 pad slots (k >= 27), ws[0] each.
__device__ __forceinline__ void conv_w_slots(int* ws, int i) {
  const int t = i >> 5, c = i & (NF - 1);
  ws[0] = i < NCONV ? wf_slot(t, c) : wf_slot(27 + ((i - NCONV) >> 5), c);
  ws[1] = wf_slot(t + 9, c);
  ws[2] = wf_slot(t + 18, c);
}
// wf: the weight fragments (conv_w_store, pad slots zeroed), cb: [32] fp32 biases
__device__ __forceinline__ void conv_setup(ConvFrag& f, const uint16_t* wf, const float* cb, int lane) {
  const int kg = lane >> 4, r = lane & 15;
  f.w[0] = ld_frag(wf + lane * 8);
  f.w[1] = ld_frag(wf + (64 + lane) * 8);
  f.bias[0] = cb[r];
  f.bias[1] = cb[16 + r];
  f.lbase = 4 * (((r >> 2) * XR + ((r >> 1) & 1)) * IMG + (r & 1));
#pragma unroll
  for (int i = 0; i < 2; ++i)
    f.tb[i] = kg == 0 ? gather_word(0, i) : kg == 1 ? gather_word(1, i) : kg == 2 ? gather_word(2, i) : gather_word(3, i);
#pragma unroll
  for (int p = 0; p < 4; ++p)
    f.sel[p] = kg == 0 ? pair_sel(0, p) : kg == 1 ? pair_sel(1, p) : kg == 2 ? pair_sel(2, p) : pair_sel(3, p);
}
// emit(image base, image offset, pl, channel, pooled_bf16, code) for every pooled output of the
// slice; the image is base + offset: base and pl are wave-uniform, offset = lane >> 4 and the
// channel depend on the lane only
// One row tile: the A fragment (8 LDS gathers, hi/lo split), then per channel half nt one
// MFMA and one bias / ReLU / pool / argmax epilogue.  HALF: only the channel half h (a
// wave-uniform runtime value) -- the two halves of a tile share nothing but the A fragment,
// so a tile split over two waves gives the same bits as one built by a single wave.
// rt (wave-uniform): windows wi = 4 rt .. 4 rt + 3 = position pl = rt >> (lg - 2), images
// b0 .. b0 + 3 with b0 = 4 rt mod 2^lg (lg >= 2: a tile never straddles two positions)
template <bool HALF, class Emit>
__device__ __forceinline__ void conv_tile(const ConvFrag& f, const float* xs, int p0, int r0, int lg, int rt, int h,
                                          int lane, Emit&& emit) {
  const int pl = rt >> (lg - 2), b0 = (4 * rt) & ((1 << lg) - 1);
  u32x4v at;
  {
    const int pos = p0 + pl, py = pos / PO, px = pos - py * PO;
    const char* base = reinterpret_cast<const char*>(xs + ((b0 * XR + 2 * py - r0) * IMG + 2 * px)) + f.lbase;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      v[j] = *reinterpret_cast<const float*>(base + ((f.tb[j >> 2] >> (8 * (j & 3))) & 0xffu));
    // x = hi + lo in bf16, a pair at a time: elementwise the values of f2bf / bf16_lo
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const f32x2v v2 = {v[2 * p], v[2 * p + 1]};
      const uint32_t hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(v2, bf16x2v));
      const f32x2v hf = {__uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u)};
      const uint32_t lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(v2 - hf, bf16x2v));
      at[p] = __builtin_amdgcn_perm(hi, lo, f.sel[p]);
    }
  }
  const bf16x8 a = __builtin_bit_cast(bf16x8, at);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int plo = pl, bo = lane >> 4;
  auto epilogue = [&](const f32x4& cc, float bias, int ch0) __attribute__((always_inline)) {
    float best = fmaxf(cc[0] + bias, 0.f);
    int arg = 0;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      const float v = fmaxf(cc[j] + bias, 0.f);
      arg = v > best ? j : arg;
      best = fmaxf(best, v);
    }
    emit(b0, bo, plo, ch0 + (lane & 15), f2bf(best), (uint8_t)(arg | (best > 0.f ? 4 : 0)));
  };
  if constexpr (HALF) {
    const bf16x8 w = h ? f.w[1] : f.w[0];
    epilogue(mfma16(a, w, zero), h ? f.bias[1] : f.bias[0], 16 * h);
  } else {
    const f32x4 c0 = mfma16(a, f.w[0], zero);
    const f32x4 c1 = mfma16(a, f.w[1], zero);
    epilogue(c0, f.bias[0], 0);
    epilogue(c1, f.bias[1], 16);
  }
}
// The slice's row tiles over the block's NW waves.  SPLIT = false: round-robin, whole tiles
// (with 12 tiles on 8 waves four waves build two, four build one).  SPLIT = true: whole tiles
// for the full rounds, the leftover tiles split by channel half over twice as many waves
// (12 tiles on 8 waves: one tile plus one half tile each).  wave: wave-uniform (readfirstlane).
template <int NW, bool SPLIT, class Emit>
__device__ __forceinline__ void conv_pool(const ConvFrag& f, const float* xs, int p0, int np, int r0, int lg,
                                          int wave, int lane, Emit&& emit) {
  const int nrt = (np << lg) >> 2;  // np positions x 2^lg images / 4 windows per tile
  const int nfull = SPLIT ? nrt / NW * NW : nrt;
  for (int rt = wave; rt < nfull; rt += NW) conv_tile<false>(f, xs, p0, r0, lg, rt, 0, lane, emit);
  if constexpr (SPLIT)
    for (int ht = wave; ht < 2 * (nrt - nfull); ht += NW)
      conv_tile<true>(f, xs, p0, r0, lg, nfull + (ht >> 1), ht & 1, lane, emit);
}

// ---- argmax codes pre-decoded for the conv gradient ------------------------------------
// The backward's conv gradient needs of a code cd = arg | on << 2 (conv_tile) the byte offset
// of the window's argmax pixel, ((cd >> 1) & 1) * IMG * 4 + (cd & 1) * 4, and the ReLU mask.
// Decoded per (image, position) pair in the gradient loop that was ~12 VALU instructions in a
// VALU-issue-bound phase; the waves that stage the codes translate them once instead, into a
// 16-bit entry per code: low byte the offset (0, 4, 112, 116), high byte 0xFF when the unit
// was on, 0x00 when off -- read back as an unsigned and a signed byte, the offset and an
// all-ones / zero mask arrive without any decoding.  Four codes (one word) take four byte
// permutes: two table look-ups with the code bytes as selectors, two interleaves.
constexpr int CGE_BYTES = 2;  // bytes per entry
constexpr uint32_t CGE_OFFS = (4u << 8) | ((uint32_t)(IMG * 4) << 16) | ((uint32_t)(IMG * 4 + 4) << 24);
static_assert(IMG * 4 + 4 < 256, "entry offsets fit a byte");
__device__ __forceinline__ void code_entries(uint32_t w, uint32_t& e01, uint32_t& e23) {
  const uint32_t sel = w & 0x07070707u;  // (only bits 0-2 of a code mean anything)
  const uint32_t offs = __builtin_amdgcn_perm(CGE_OFFS, CGE_OFFS, sel);  // codes 4-7: the offsets of 0-3
  const uint32_t mask = __builtin_amdgcn_perm(0xffffffffu, 0u, sel);     // codes 4-7: on
  e01 = __builtin_amdgcn_perm(mask, offs, 0x05010400u);
  e23 = __builtin_amdgcn_perm(mask, offs, 0x07030602u);
}

// ---- fixed-point cross-block sums, DPP row reductions, small MFMA, SGD-or-keep ----------
constexpr float HSCALE = 4294967296.f;          // 2^32
constexpr double HINV = 1.0 / 4294967296.0;
constexpr float CSCALE = 1099511627776.f;       // 2^40
constexpr double CINV = 1.0 / 1099511627776.0;

// |v * scale| < 2^54: a sum of up to 512 such terms (57 slices x 8 ranks) stays inside int64.
// Anything else -- NaN, inf, a diverged partial -- is not representable: it is counted as 0
// and raises the sticky ctrl->bad flag, and the step reports loss = NaN from then on (the
// fp32 engines would show the NaN; a wrapped integer must not turn it into finite garbage)
constexpr float FIX_LIMIT = 18014398509481984.f;  // 2^54
__device__ __forceinline__ long long to_fix(float v, float scale, int* bad) {
  const float q = v * scale;
  if (!(fabsf(q) < FIX_LIMIT)) {
    __hip_atomic_fetch_or(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return 0;
  }
  return (long long)__builtin_rintf(q);
}
// fixed point -> float as (q >> 24) * 2^24 + (q & (2^24 - 1)) in one fma: f32 only (the
// former (float)((double)q * inv) took ~6 half-rate f64 instructions per value, and the
// head converts 8 per thread).  Both parts are exact floats for |q| < 2^48 (the signed
// high part is arithmetic-shifted, the low part has 24 bits), so the fma rounds ONCE: the
// correctly rounded value, negative q included (round 5 split at 2^32 and rounded the
// unsigned low word first: q = -5 decoded to 0).  inv is a power of two.
__device__ __forceinline__ float from_fix(long long q, double inv) {
  const float fi = (float)inv;
  return fmaf((float)(q >> 24), fi * 16777216.f, (float)(int)(q & 0xFFFFFF) * fi);
}
// The same value without the 64-bit conversion.  hipcc expands (float)(int64) into ~13 VALU
// instructions, two 64-bit shifts among them, per value; when q >> 24 fits an int32 --
// |q| < 2^55: every dense-1 sum and conv gradient short of divergence -- that high part is one
// v_alignbit_b32 and converts with v_cvt_f32_i32 to the same correctly rounded float.
// fix_narrow: bits 63 .. 55 of q are copies of one sign bit.
__device__ __forceinline__ bool fix_narrow(long long q) {
  return (unsigned)(((int)(q >> 32) >> 23) + 1) < 2u;
}
__device__ __forceinline__ float from_fix_narrow(long long q, double inv) {
  const float fi = (float)inv;
  const int h = (int)__builtin_amdgcn_alignbit((uint32_t)((unsigned long long)q >> 32), (uint32_t)q, 24);
  return fmaf((float)h, fi * 16777216.f, (float)(int)((uint32_t)q & 0xFFFFFFu) * fi);
}
// N values per lane: the narrow form when every value of every lane of the wave fits (one
// ballot, a scalar branch), else from_fix as it stands -- for every int64 the bits of from_fix.
// (A per-lane select between the two forms compiles back into the 64-bit sequence.)  Call it
// where whole waves arrive together (the ballot covers the active lanes).
template <int N>
__device__ __forceinline__ void from_fix_wave(float (&out)[N], const long long (&q)[N], double inv) {
  bool wide = false;
#pragma unroll
  for (int i = 0; i < N; ++i) wide |= !fix_narrow(q[i]);
  if (__builtin_amdgcn_ballot_w64(wide) == 0ull) {
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = from_fix_narrow(q[i], inv);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = from_fix(q[i], inv);
  }
}

__device__ __forceinline__ void atomic_add_i64(long long* p, long long v) {
  __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}

// Reductions over the 16 lanes of a DPP row (one MFMA output column group) on DPP moves:
// quad swaps, then half-row and row mirrors; every lane ends with the row's result, and
// the combination order is fixed (deterministic).
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ int dppi(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
constexpr int DPP_QSWAP1 = 0xB1, DPP_QSWAP2 = 0x4E, DPP_HMIRROR = 0x141, DPP_MIRROR = 0x140;
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dppf<DPP_QSWAP1>(v));
  v = fmaxf(v, dppf<DPP_QSWAP2>(v));
  v = fmaxf(v, dppf<DPP_HMIRROR>(v));
  return fmaxf(v, dppf<DPP_MIRROR>(v));
}
// (row16_sum: damd_common.h, the same DPP sequence, shared with the GEMM epilogues)
__device__ __forceinline__ int row16_min(int v) {
  v = min(v, dppi<DPP_QSWAP1>(v));
  v = min(v, dppi<DPP_QSWAP2>(v));
  v = min(v, dppi<DPP_HMIRROR>(v));
  return min(v, dppi<DPP_MIRROR>(v));
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ void sgd_or_keep(bool pend, float w, float g, float v, const Ctrl& c, float& wn,
                                            float& vn) {
  if (pend) {
    sgd_update(w, g, v, c.lr, c.momentum, c.nesterov, wn, vn);
  } else {
    wn = w;
    vn = v;
  }
}

}  // namespace convnet
}  // namespace damd
