// Elementwise and data / layout glue of the generic path: ReLU backward, pointwise
// activations, dropout, the residual add, dtype casts, the step's batch gather (which also
// clears the step's accumulators and sets the step counter) and the padded weight layouts.
// bf16 tensors move as 16-byte vectors of 8 elements; no reductions, no atomics.
#include "layer_dev.h"

namespace damd {
namespace {

__global__ __launch_bounds__(NT) void relu_bwd_k(const uint16_t* dy, const uint16_t* y, uint16_t* dz, long n8) {
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += (long)gridDim.x * NT) {
    float d[8], yv[8];
    unpack8(reinterpret_cast<const uint4*>(dy)[i], d);
    unpack8(reinterpret_cast<const uint4*>(y)[i], yv);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = yv[e] > 0.f ? d[e] : 0.f;
    reinterpret_cast<uint4*>(dz)[i] = pack8(d);
  }
}

// Pointwise activations on bf16 tensors (kind 0 relu, 1 sigmoid, 2 tanh).  The backward
// reads the stored output y: relu' = [y > 0], sigmoid' = y (1 - y), tanh' = 1 - y^2.  A
// thread owns 8 elements (one 16-byte access); the last, partial group of a length that
// is not a multiple of 8 goes element by element.
__device__ __forceinline__ float act_f(float z, int kind) {
  if (kind == 1) return 1.f / (1.f + __expf(-z));
  if (kind == 2) return tanhf(z);
  return fmaxf(z, 0.f);
}
__device__ __forceinline__ float act_df(float y, int kind) {
  if (kind == 1) return y * (1.f - y);
  if (kind == 2) return 1.f - y * y;
  return y > 0.f ? 1.f : 0.f;
}

__global__ __launch_bounds__(NT) void act_fwd_k(const uint16_t* x, uint16_t* y, long n, int kind) {
  const long n8 = (n + 7) / 8;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += (long)gridDim.x * NT) {
    if (8 * i + 8 <= n) {
      float v[8];
      unpack8(reinterpret_cast<const uint4*>(x)[i], v);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = act_f(v[e], kind);
      reinterpret_cast<uint4*>(y)[i] = pack8(v);
    } else {
      for (long j = 8 * i; j < n; ++j) y[j] = f2bf(act_f(bf2f(x[j]), kind));
    }
  }
}

__global__ __launch_bounds__(NT) void act_bwd_k(const uint16_t* dy, const uint16_t* y, uint16_t* dx, long n,
                                                int kind) {
  const long n8 = (n + 7) / 8;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += (long)gridDim.x * NT) {
    if (8 * i + 8 <= n) {
      float d[8], yv[8];
      unpack8(reinterpret_cast<const uint4*>(dy)[i], d);
      unpack8(reinterpret_cast<const uint4*>(y)[i], yv);
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] *= act_df(yv[e], kind);
      reinterpret_cast<uint4*>(dx)[i] = pack8(d);
    } else {
      for (long j = 8 * i; j < n; ++j) dx[j] = f2bf(bf2f(dy[j]) * act_df(bf2f(y[j]), kind));
    }
  }
}

// Dropout with a counter-based mask: element j of step t is kept iff
// drop_hash(key_t, j) >= rate * 2^32, key_t = mix32(seed + t * golden), t = ctrl->cur3 (the
// step's iteration, set by gather_batch).  No mask tensor and no RNG state: the backward
// regenerates the same mask from (seed, t, j), and a graph replay draws a fresh mask
// because t advances on the device.  Kept elements are scaled by 1 / (1 - rate).
// distributed_amd/engine/native_graph.py:dropout_mask_reference is the host oracle.
// (mix32: damd_common.h, shared with augment.hip)
__global__ __launch_bounds__(NT) void dropout_k(const uint16_t* x, uint16_t* y, long n, const Ctrl* ctrl,
                                                uint32_t seed, uint32_t thr, float scale) {
  const uint32_t key = mix32(seed + (uint32_t)ctrl->cur3 * 0x9e3779b9u);
  const long n8 = (n + 7) / 8;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += (long)gridDim.x * NT) {
    if (8 * i + 8 <= n) {
      float v[8];
      unpack8(reinterpret_cast<const uint4*>(x)[i], v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t h = mix32(mix32((uint32_t)(8 * i + e) ^ key) + key);
        v[e] = h >= thr ? v[e] * scale : 0.f;
      }
      reinterpret_cast<uint4*>(y)[i] = pack8(v);
    } else {
      for (long j = 8 * i; j < n; ++j) {
        const uint32_t h = mix32(mix32((uint32_t)j ^ key) + key);
        y[j] = f2bf(h >= thr ? bf2f(x[j]) * scale : 0.f);
      }
    }
  }
}

__global__ __launch_bounds__(NT) void add_bf16_k(const uint16_t* a, const uint16_t* b, uint16_t* o, long n8) {
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n8; i += (long)gridDim.x * NT) {
    float x[8], y[8];
    unpack8(reinterpret_cast<const uint4*>(a)[i], x);
    unpack8(reinterpret_cast<const uint4*>(b)[i], y);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] += y[e];
    reinterpret_cast<uint4*>(o)[i] = pack8(x);
  }
}

__global__ __launch_bounds__(NT) void cast_f32_bf16_k(const float* x, uint16_t* y, long n) {
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) y[i] = f2bf(x[i]);
}

__global__ __launch_bounds__(NT) void cast_bf16_f32_k(const uint16_t* x, float* y, long n) {
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) y[i] = bf2f(x[i]);
}

__global__ __launch_bounds__(NT) void cast_u8_bf16_k(const uint8_t* x, float scale, uint16_t* y, long n) {
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < n; i += (long)gridDim.x * NT)
    y[i] = f2bf((float)x[i] * scale);
}

__global__ __launch_bounds__(NT) void gather_batch_k(const void* __restrict__ x, int x_u8, float scale,
                                                     const int32_t* __restrict__ labels, Ctrl* __restrict__ ctrl,
                                                     int per, int HW, int Cin, int Cp, uint16_t* __restrict__ xb,
                                                     int32_t* __restrict__ yb, uint4* __restrict__ zero, long nz16,
                                                     uint4* __restrict__ zero2, long nz16b, PadCastJob pc) {
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < nz16; i += (long)gridDim.x * NT) zero[i] = uint4{0u, 0u, 0u, 0u};
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < nz16b; i += (long)gridDim.x * NT) zero2[i] = uint4{0u, 0u, 0u, 0u};
  // a layer's padded bf16 weight copy, element for element as pad_cast_k: a thread's first
  // element is loaded here and stored when the thread's gather work is done (the load's
  // latency hides under it; loading and storing up front cost the launch ~2 us)
  const long pc_total = pc.src ? (long)pc.R * pc.C1p * pc.C2p : 0;
  const long gt = blockIdx.x * (long)NT + threadIdx.x;
  auto pc_src = [&](long i) -> const float* {
    const int c2 = (int)(i % pc.C2p);
    const long t = i / pc.C2p;
    const int c1 = (int)(t % pc.C1p), r = (int)(t / pc.C1p);
    return c1 < pc.C1 && c2 < pc.C2 ? pc.src + ((long)r * pc.C1 + c1) * pc.C2 + c2 : nullptr;
  };
  float pcf = 0.f;
  if (gt < pc_total) {
    const float* p = pc_src(gt);
    pcf = p ? *p : 0.f;
  }
  auto pc_finish = [&]() {
    if (gt >= pc_total) return;
    pc.dst[gt] = f2bf(pcf);
    for (long i = gt + (long)gridDim.x * NT; i < pc_total; i += (long)gridDim.x * NT) {
      const float* p = pc_src(i);
      pc.dst[i] = p ? f2bf(*p) : (uint16_t)0;
    }
  };
  const long base = (long)ctrl->cursor * ctrl->global_batch + ctrl->row0;
  const int n = ctrl->nsamples;
  const bool wrap = ctrl->wrap > 0;  // benchmark mode: the epoch wraps, every row is real
  if (blockIdx.x == 0 && threadIdx.x == 0) ctrl->cur3 = ctrl->iterations + 1;  // this step's t (opt_step)
  if (Cp == 4 && Cin == 3 && x_u8 && HW % 4 == 0) {
    // RGB uint8 rows -> packed 4-channel bf16: one thread per 4 pixels of one row, the 12
    // source bytes as three aligned dword loads (byte loads moved 64 B per wave
    // instruction), two 16-byte stores
    const long total = (long)per * HW / 4;
    for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
      const long pr = 4 * i;
      const int p = (int)(pr % HW), r = (int)(pr / HW);
      const bool valid = wrap || base + r < n;
      const long row = valid ? (base + r) % n : 0;
      uint32_t w[3] = {0u, 0u, 0u};
      if (valid) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>((const uint8_t*)x + (row * HW + p) * 3);
        w[0] = src[0];
        w[1] = src[1];
        w[2] = src[2];
      }
      float v[16];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int b = 3 * k + c;
          v[4 * k + c] = (float)((w[b >> 2] >> (8 * (b & 3))) & 0xffu) / scale;
        }
        v[4 * k + 3] = 0.f;
      }
      if (p == 0) yb[r] = valid ? labels[row] : -1;
      reinterpret_cast<uint4*>(xb)[2 * i] = pack8(v);
      reinterpret_cast<uint4*>(xb)[2 * i + 1] = pack8(v + 8);
    }
    pc_finish();
    return;
  }
  if (Cp == 4) {
    // packed-tap stem input (4 channels): one thread per 2 pixels, one 16-byte store
    const long total = (long)per * HW / 2;
    for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
      float v[8];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const long pr = 2 * i + h;
        const int p = (int)(pr % HW), r = (int)(pr / HW);
        const bool valid = wrap || base + r < n;
        const long row = valid ? (base + r) % n : 0;
        const long si = (row * HW + p) * Cin;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          v[4 * h + c] = 0.f;
          if (c < Cin && valid)
            v[4 * h + c] = x_u8 ? (float)((const uint8_t*)x)[si + c] / scale : ((const float*)x)[si + c];
        }
        if (p == 0) yb[r] = valid ? labels[row] : -1;
      }
      reinterpret_cast<uint4*>(xb)[i] = pack8(v);
    }
    pc_finish();
    return;
  }
  // one thread per 8 (padded) channels of one pixel: one 16-byte store
  const int cg = Cp / 8;
  const long total = (long)per * HW * cg;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c8 = (int)(i % cg);
    const long pr = i / cg;
    const int p = (int)(pr % HW), r = (int)(pr / HW);
    // rows past the end of a short final batch: zero image, label -1 (masked downstream)
    const bool valid = wrap || base + r < n;
    const long row = valid ? (base + r) % n : 0;
    const long si = (row * HW + p) * Cin;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c8 * 8 + e;
      v[e] = 0.f;
      if (c < Cin && valid)
        v[e] = x_u8 ? (float)((const uint8_t*)x)[si + c] / scale : ((const float*)x)[si + c];
    }
    reinterpret_cast<uint4*>(xb)[i] = pack8(v);
    if (p == 0 && c8 == 0) yb[r] = valid ? labels[row] : -1;
  }
  pc_finish();
}

__global__ __launch_bounds__(NT) void pad_cast_k(const float* src, int R, int C1, int C2, int C1p, int C2p,
                                                 uint16_t* dst) {
  const long total = (long)R * C1p * C2p;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c2 = (int)(i % C2p);
    const long t = i / C2p;
    const int c1 = (int)(t % C1p), r = (int)(t / C1p);
    dst[i] = (c1 < C1 && c2 < C2) ? f2bf(src[((long)r * C1 + c1) * C2 + c2]) : (uint16_t)0;
  }
}

__global__ __launch_bounds__(NT) void unpad_add_k(const float* src, int R, int C1, int C2, int C1p, int C2p,
                                                  float* dst) {
  const long total = (long)R * C1 * C2;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c2 = (int)(i % C2);
    const long t = i / C2;
    const int c1 = (int)(t % C1), r = (int)(t / C1);
    dst[i] += src[((long)r * C1p + c1) * C2p + c2];
  }
}

}  // namespace

hipError_t relu_bwd(const uint16_t* dy, const uint16_t* y, uint16_t* dz, long n, hipStream_t s) {
  if (n % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(relu_bwd_k, dim3(grid_for(n / 8)), dim3(NT), 0, s, dy, y, dz, n / 8);
  return hipGetLastError();
}

hipError_t act_fwd(const uint16_t* x, uint16_t* y, long n, int kind, hipStream_t s) {
  if (kind < 0 || kind > 2 || n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(act_fwd_k, dim3(grid_for((n + 7) / 8)), dim3(NT), 0, s, x, y, n, kind);
  return hipGetLastError();
}

hipError_t act_bwd(const uint16_t* dy, const uint16_t* y, uint16_t* dx, long n, int kind, hipStream_t s) {
  if (kind < 0 || kind > 2 || n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(act_bwd_k, dim3(grid_for((n + 7) / 8)), dim3(NT), 0, s, dy, y, dx, n, kind);
  return hipGetLastError();
}

hipError_t dropout(const uint16_t* x, uint16_t* y, long n, const Ctrl* ctrl, uint32_t seed, float rate,
                   hipStream_t s) {
  if (!(rate >= 0.f && rate < 1.f) || n <= 0) return hipErrorInvalidValue;
  const uint32_t thr = (uint32_t)fmin((double)rate * 4294967296.0, 4294967295.0);
  hipLaunchKernelGGL(dropout_k, dim3(grid_for((n + 7) / 8)), dim3(NT), 0, s, x, y, n, ctrl, seed, thr,
                     1.f / (1.f - rate));
  return hipGetLastError();
}

hipError_t add_bf16(const uint16_t* a, const uint16_t* b, uint16_t* out, long n, hipStream_t s) {
  if (n % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(add_bf16_k, dim3(grid_for(n / 8)), dim3(NT), 0, s, a, b, out, n / 8);
  return hipGetLastError();
}

hipError_t cast_f32_bf16(const float* x, uint16_t* y, long n, hipStream_t s) {
  hipLaunchKernelGGL(cast_f32_bf16_k, dim3(grid_for(n)), dim3(NT), 0, s, x, y, n);
  return hipGetLastError();
}

hipError_t cast_bf16_f32(const uint16_t* x, float* y, long n, hipStream_t s) {
  hipLaunchKernelGGL(cast_bf16_f32_k, dim3(grid_for(n)), dim3(NT), 0, s, x, y, n);
  return hipGetLastError();
}

hipError_t cast_u8_bf16(const uint8_t* x, float scale, uint16_t* y, long n, hipStream_t s) {
  hipLaunchKernelGGL(cast_u8_bf16_k, dim3(grid_for(n)), dim3(NT), 0, s, x, scale, y, n);
  return hipGetLastError();
}

hipError_t gather_batch(const void* x, int x_u8, float scale, const int32_t* labels, Ctrl* ctrl, int per,
                        int HW, int Cin, int Cp, uint16_t* xb, int32_t* yb, hipStream_t s, void* zero, long zero_bytes,
                        void* zero2, long zero2_bytes, PadCastJob pc) {
  if (pc.src && (!pc.dst || pc.R < 1 || pc.C1 < 1 || pc.C2 < 1 || pc.C1p < pc.C1 || pc.C2p < pc.C2))
    return hipErrorInvalidValue;
  if (Cp % 8 && !(Cp == 4 && Cin <= 4 && HW % 2 == 0)) return hipErrorInvalidValue;
  // the RGB uint8 path (the kernel's first branch) reads x as dwords
  if (Cp == 4 && Cin == 3 && x_u8 && HW % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 4) return hipErrorInvalidValue;
  for (int k = 0; k < 2; ++k) {
    const void* z = k ? zero2 : zero;
    const long nb = k ? zero2_bytes : zero_bytes;
    if (nb < 0 || nb % 16 || (nb > 0 && (z == nullptr || reinterpret_cast<uintptr_t>(z) % 16)))
      return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(gather_batch_k, dim3(grid_for((long)per * HW * Cp / 8)), dim3(NT), 0, s, x, x_u8, scale, labels,
                     ctrl, per, HW, Cin, Cp, xb, yb, static_cast<uint4*>(zero), zero_bytes / 16,
                     static_cast<uint4*>(zero2), zero2_bytes / 16, pc);
  return hipGetLastError();
}

hipError_t pad_cast(const float* src, int R, int C1, int C2, int C1p, int C2p, uint16_t* dst, hipStream_t s) {
  hipLaunchKernelGGL(pad_cast_k, dim3(grid_for((long)R * C1p * C2p)), dim3(NT), 0, s, src, R, C1, C2, C1p, C2p, dst);
  return hipGetLastError();
}

hipError_t unpad_add(const float* src, int R, int C1, int C2, int C1p, int C2p, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(unpad_add_k, dim3(grid_for((long)R * C1 * C2)), dim3(NT), 0, s, src, R, C1, C2, C1p, C2p, dst);
  return hipGetLastError();
}

}  // namespace damd
