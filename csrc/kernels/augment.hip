// Input augmentation for the graph engines: ZeroPadding2D / RandomCrop / RandomFlip chains at
// the model input as one gather (layer_ops.h augment has the contract).
//
// Grid (blocks per sample, B): the sample is blockIdx.y, so everything drawn per sample --
// flip bits and crop offsets of every stage -- depends on kernel arguments, blockIdx.y and
// two uniform loads (ctrl->cur3, ctrl->row0) only: it is computed once per block, in scalar
// registers, ahead of the pixel loop.  The stage table arrives by value in the kernel
// arguments; the stage loops are fully unrolled so a stage's draws stay in named registers.
// A thread moves one pixel chunk per iteration (V = 8 bytes for a pixel pitch of 8 bytes
// mod 16, else 16 bytes): consecutive threads write consecutive chunks, and read
// consecutive (or, under a left-right flip, pixel-reversed) chunks of a source row.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "damd_common.h"
#include "layer_ops.h"

namespace damd {
namespace {

constexpr int AUG_NT = 256;

template <typename V>
__global__ __launch_bounds__(AUG_NT) void augment_k(const V* __restrict__ x, V* __restrict__ y,
                                                    const int32_t* __restrict__ labels,
                                                    const Ctrl* __restrict__ ctrl, AugTable tab, int H, int W, int Ho,
                                                    int Wo, int chunks, int training) {
  const int b = blockIdx.y;
  const bool valid = labels[b] >= 0;
  const uint32_t t = (uint32_t)ctrl->cur3, g = (uint32_t)(ctrl->row0 + b);
  // per-sample draws (d0 / d1 = flip left-right / up-down, crop offset y / x, pad top / left)
  // and every stage's input size, walking the chain forward from H x W
  int d0[AUG_MAX_STAGES], d1[AUG_MAX_STAGES], ih[AUG_MAX_STAGES], iw[AUG_MAX_STAGES];
  int h = H, w = W;
#pragma unroll
  for (int s = 0; s < AUG_MAX_STAGES; ++s) {
    d0[s] = d1[s] = 0;
    ih[s] = h, iw[s] = w;
    if (s >= tab.n) continue;
    const AugStage& st = tab.st[s];
    const uint32_t key = mix32(st.seed + t * 0x9e3779b9u);
    const uint32_t r = mix32(mix32(g ^ key) + key);
    if (st.kind == AUG_FLIP) {
      d0[s] = training && (st.p[0] & 1) ? (int)(r >> 31) : 0;
      d1[s] = training && (st.p[0] & 2) ? (int)((r >> 30) & 1u) : 0;
    } else if (st.kind == AUG_CROP) {
      const int ry = h - st.p[0], rx = w - st.p[1];  // (host: >= 0)
      d0[s] = training ? (int)(r % (uint32_t)(ry + 1)) : ry / 2;
      d1[s] = training ? (int)(mix32(r + key) % (uint32_t)(rx + 1)) : rx / 2;
      h = st.p[0], w = st.p[1];
    } else {
      d0[s] = st.p[0];
      d1[s] = st.p[2];
      h += st.p[0] + st.p[1], w += st.p[2] + st.p[3];
    }
  }
  const int per = Ho * Wo * chunks;  // (host: below 2^30)
  const V* xs = x + (long)b * H * W * chunks;
  V* ys = y + (long)b * per;
  for (int i = blockIdx.x * AUG_NT + threadIdx.x; i < per; i += gridDim.x * AUG_NT) {
    const int pix = i / chunks, ch = i - pix * chunks;
    int oy = pix / Wo, ox = pix - oy * Wo;
    bool zero = !valid;
#pragma unroll
    for (int s = AUG_MAX_STAGES - 1; s >= 0; --s) {
      if (s >= tab.n) continue;
      const AugStage& st = tab.st[s];
      if (st.kind == AUG_FLIP) {
        if (d0[s]) ox = iw[s] - 1 - ox;
        if (d1[s]) oy = ih[s] - 1 - oy;
      } else if (st.kind == AUG_CROP) {
        oy += d0[s];
        ox += d1[s];
      } else {
        oy -= d0[s];
        ox -= d1[s];
        zero = zero || (unsigned)oy >= (unsigned)ih[s] || (unsigned)ox >= (unsigned)iw[s];
      }
    }
    // (a consistent table keeps a non-zero pixel inside the image; the check costs nothing)
    zero = zero || (unsigned)oy >= (unsigned)H || (unsigned)ox >= (unsigned)W;
    V v{};
    if (!zero) v = xs[((long)oy * W + ox) * chunks + ch];
    ys[i] = v;
  }
}

// the table describes a chain H x W -> ... -> Ho x Wo
bool table_ok(const AugTable& tab, int H, int W, int Ho, int Wo) {
  if (tab.n < 1 || tab.n > AUG_MAX_STAGES) return false;
  long h = H, w = W;
  for (int s = 0; s < tab.n; ++s) {
    const int32_t* p = tab.st[s].p;
    if (tab.st[s].kind == AUG_FLIP) {
      if (p[0] < 1 || p[0] > 3) return false;
    } else if (tab.st[s].kind == AUG_CROP) {
      if (p[0] < 1 || p[1] < 1 || p[0] > h || p[1] > w) return false;
      h = p[0], w = p[1];
    } else if (tab.st[s].kind == AUG_PAD) {
      for (int k = 0; k < 4; ++k)
        if (p[k] < 0 || p[k] > (1 << 20)) return false;
      h += p[0] + p[1], w += p[2] + p[3];
    } else {
      return false;
    }
    if (h > (1 << 20) || w > (1 << 20)) return false;
  }
  return h == Ho && w == Wo;
}

}  // namespace

hipError_t augment(const uint16_t* x, uint16_t* y, const int32_t* labels, const Ctrl* ctrl, const AugTable* tab, int B,
                   int H, int W, int Ho, int Wo, int Cp, int training, hipStream_t s) {
  if (!x || !y || !labels || !ctrl || !tab || x == y) return hipErrorInvalidValue;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || Ho < 1 || Wo < 1 || Cp < 4 || Cp % 4) return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(x) % 16 || reinterpret_cast<uintptr_t>(y) % 16) return hipErrorInvalidValue;
  if (!table_ok(*tab, H, W, Ho, Wo)) return hipErrorInvalidValue;
  const bool wide = Cp % 8 == 0;
  const int chunks = wide ? Cp / 8 : Cp / 4;
  if ((long)H * W * chunks >= (1L << 30) || (long)Ho * Wo * chunks >= (1L << 30)) return hipErrorInvalidValue;
  const int per = Ho * Wo * chunks;
  const dim3 grid((unsigned)std::min((per + AUG_NT - 1) / AUG_NT, 64), (unsigned)B);
  if (wide)
    hipLaunchKernelGGL(augment_k<uint4>, grid, dim3(AUG_NT), 0, s, reinterpret_cast<const uint4*>(x),
                       reinterpret_cast<uint4*>(y), labels, ctrl, *tab, H, W, Ho, Wo, chunks, training);
  else
    hipLaunchKernelGGL(augment_k<uint2>, grid, dim3(AUG_NT), 0, s, reinterpret_cast<const uint2*>(x),
                       reinterpret_cast<uint2*>(y), labels, ctrl, *tab, H, W, Ho, Wo, chunks, training);
  return hipGetLastError();
}

}  // namespace damd
