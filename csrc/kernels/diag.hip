// Diagnostic kernels (scheduling probes, scripts/probe_graph_branches.py): a grid of blocks
// that each hold their CU for `ticks` s_memrealtime ticks (100 MHz), block 0 recording its
// start / end.  Used to see which captured-graph branches the HIP runtime lets run
// concurrently (e.g. a gradient all-reduce node beside the backward kernels).
#include <hip/hip_runtime.h>

#include "convnet_dev.h"

namespace damd {
namespace {

__global__ __launch_bounds__(64) void spin_stamp_k(long long ticks, unsigned long long* __restrict__ out, int slot) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long t = t0;
  while ((long long)(t - t0) < ticks) {
    __builtin_amdgcn_s_sleep(2);
    t = __builtin_amdgcn_s_memrealtime();
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && out != nullptr) {
    out[2 * slot] = t0;
    out[2 * slot + 1] = t;
  }
}

// Test-only pair (tests/test_convnet_fwd_lds_poison_gpu.py): LDS is not cleared between
// workgroups, so a kernel that reads a word nobody staged sees what an earlier workgroup on
// the CU left there.  lds_poison_k fills each workgroup's whole LDS (one workgroup per CU at
// this size) with 0x7FC07FC0 -- a quiet NaN as fp32 and as two bf16 --; lds_count_k counts
// that pattern in LDS it never wrote (0: this device does not retain LDS contents).
constexpr int LDS_ALL = 160 * 1024, LDS_WORDS = LDS_ALL / 4;
constexpr unsigned LDS_POISON = 0x7FC07FC0u;

__global__ __launch_bounds__(1024) void lds_poison_k() {
  extern __shared__ __attribute__((aligned(16))) unsigned lds_words[];
  for (int i = threadIdx.x; i < LDS_WORDS; i += 1024) lds_words[i] = LDS_POISON;
  // (nothing reads the words in this kernel: the asm keeps the stores, and waits for them)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(1024) void lds_count_k(unsigned long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned lds_words[];
  unsigned n = 0;
  for (int i = threadIdx.x; i < LDS_WORDS; i += 1024) n += lds_words[i] == LDS_POISON ? 1u : 0u;
  if (n) __hip_atomic_fetch_add(out, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Test-only (tests/test_fixpoint_decode_gpu.py): the step kernels' two fixed-point decodes on the
// same inputs -- from_fix_wave as the backward's h phase calls it (4 consecutive values per
// thread, one wave-uniform test per wave) into `fast`, from_fix into `ref`.  n: a multiple of 4.
template <int SCALE>  // 0: HINV (dense-1 sums), 1: CINV (conv gradient)
__global__ __launch_bounds__(256) void fix_decode_k(const long long* __restrict__ q, float* __restrict__ fast,
                                                    float* __restrict__ ref, int n) {
  constexpr double inv = SCALE == 0 ? convnet::HINV : convnet::CINV;
  const int i = 4 * (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  long long v[4];
  float f[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = q[i + j];
  convnet::from_fix_wave(f, v, inv);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    fast[i + j] = f[j];
    ref[i + j] = convnet::from_fix(v[j], inv);
  }
}

hipError_t lds_all(const void* k) {
  return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_ALL);
}

}  // namespace

hipError_t lds_poison(int blocks, hipStream_t s) {
  if (blocks < 1 || blocks > 65536) return hipErrorInvalidValue;
  const hipError_t e = lds_all((const void*)lds_poison_k);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lds_poison_k, dim3(blocks), dim3(1024), LDS_ALL, s);
  return hipGetLastError();
}

// adds to *out the number of poison words the blocks found in LDS they did not write
hipError_t lds_count(int blocks, unsigned long long* out, hipStream_t s) {
  if (blocks < 1 || blocks > 65536 || out == nullptr) return hipErrorInvalidValue;
  const hipError_t e = lds_all((const void*)lds_count_k);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lds_count_k, dim3(blocks), dim3(1024), LDS_ALL, s, out);
  return hipGetLastError();
}

// fast[i] = from_fix_wave, ref[i] = from_fix of q[i], i < n (n a multiple of 4); scale 0: 2^-32, 1: 2^-40
hipError_t fix_decode(const long long* q, float* fast, float* ref, int n, int scale, hipStream_t s) {
  if (q == nullptr || fast == nullptr || ref == nullptr || n < 4 || n % 4 != 0 || scale < 0 || scale > 1)
    return hipErrorInvalidValue;
  const dim3 grid((n / 4 + 255) / 256);
  if (scale == 0) hipLaunchKernelGGL(fix_decode_k<0>, grid, dim3(256), 0, s, q, fast, ref, n);
  else hipLaunchKernelGGL(fix_decode_k<1>, grid, dim3(256), 0, s, q, fast, ref, n);
  return hipGetLastError();
}

hipError_t spin_stamp(long long ticks, int blocks, unsigned long long* out, int slot, hipStream_t s) {
  if (blocks < 1 || ticks < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(spin_stamp_k, dim3(blocks), dim3(64), 0, s, ticks, out, slot);
  return hipGetLastError();
}

}  // namespace damd
