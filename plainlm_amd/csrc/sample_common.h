// What the sampling kernels share (DESIGN.md sections 13 and 15): the order-preserving key of a bf16 logit, the fixed-point weight of a
// logit below its row maximum, and the block-wide integer reductions.  sample.hip draws a token with them; spec.hip rebuilds the very
// weights a token was drawn with, so the two files must not carry copies that could drift apart.
#pragma once

#include <cmath>

#include "plm_device.h"

#define SMP_THREADS 1024
#define SMP_WAVES (SMP_THREADS / PLM_WAVE)
#define SMP_KEY_LO 0x0080u   // key of the most negative finite bf16 (-inf is 0x007F)
#define SMP_KEY_HI 0xFF7Fu   // key of the largest finite bf16 (+inf is 0xFF80)
#define SMP_NONE (~0ull)

typedef unsigned long long smp_u64;

// bf16 bits -> key: a larger value has a larger key, equal values have equal keys, NaN and the infinities map to 0
__device__ __forceinline__ unsigned smp_key(unsigned bits) {
  if (bits == 0x8000u) bits = 0u;
  const unsigned k = (bits & 0x8000u) ? (~bits & 0xFFFFu) : (bits | 0x8000u);
  return (k >= SMP_KEY_LO && k <= SMP_KEY_HI) ? k : 0u;
}
__device__ __forceinline__ float smp_value(unsigned k) {
  const unsigned bits = (k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu);
  return __uint_as_float(bits << 16);
}
// Weight of a logit d = x - x_max <= 0 below the maximum, as fixed point: exp(d / tau) = 2^(d * c) with c = log2(e) / tau rounded once
// on the host, through v_exp_f32 (1 ulp; 2^0 = 1 exactly).  The argument carries two roundings, so a weight is off by |d / tau| * 1.2e-7
// of itself at most; the softmax mean of |d / tau| is at most ln V, so any sum of weights is within 1.2e-7 ln V of Z of the exact one
// (1.3e-6 at V = 65,544, under the 4e-6 the draw is held to).  A function of the key alone, so equal logits have equal weights.
// (expf(d / tau) cost about sixty VALU instructions per column: 0.02 ms for every pass over 50,280 columns that takes an exponential.)
static constexpr float SMP_LOG2E = 1.4426950408889634f;
__device__ __forceinline__ smp_u64 smp_fix(float d, float c, float scale) { return (smp_u64)(__builtin_amdgcn_exp2f(d * c) * scale); }

// ---- block-wide integer reductions: every thread receives the result; two barriers each, s_part is free again on return ------------
__device__ __forceinline__ smp_u64 smp_block_sum(smp_u64 v, smp_u64* s_part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, PLM_WAVE);
  if (threadIdx.x % PLM_WAVE == 0) s_part[threadIdx.x / PLM_WAVE] = v;
  __syncthreads();
  smp_u64 t = 0;
#pragma unroll
  for (int w = 0; w < SMP_WAVES; ++w) t += s_part[w];
  __syncthreads();
  return t;
}
__device__ __forceinline__ smp_u64 smp_block_max(smp_u64 v, smp_u64* s_part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const smp_u64 t = __shfl_xor(v, o, PLM_WAVE);
    v = t > v ? t : v;
  }
  if (threadIdx.x % PLM_WAVE == 0) s_part[threadIdx.x / PLM_WAVE] = v;
  __syncthreads();
  smp_u64 m = 0;
#pragma unroll
  for (int w = 0; w < SMP_WAVES; ++w) m = s_part[w] > m ? s_part[w] : m;
  __syncthreads();
  return m;
}
// inclusive scan in thread order; total = the sum over the block
__device__ __forceinline__ smp_u64 smp_block_scan(smp_u64 v, smp_u64* s_part, smp_u64& total) {
  const int lane = threadIdx.x % PLM_WAVE, wave = threadIdx.x / PLM_WAVE;
#pragma unroll
  for (int o = 1; o < PLM_WAVE; o <<= 1) {
    const smp_u64 t = __shfl_up(v, o, PLM_WAVE);
    if (lane >= o) v += t;
  }
  if (lane == PLM_WAVE - 1) s_part[wave] = v;
  __syncthreads();
  smp_u64 base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SMP_WAVES; ++w) {
    const smp_u64 x = s_part[w];
    base += w < wave ? x : 0;
    tot += x;
  }
  __syncthreads();
  total = tot;
  return v + base;
}

// ---- host: the two launch scalars every kernel that rebuilds a weight must derive the same way -------------------------------------
// fixed point: a weight is at most 1, a sum of V of them must stay below 2^63
static inline float smp_host_scale(int64_t V) {
  int shift = 40;
  while (ldexp((double)V, shift) >= 9223372036854775808.0) --shift;
  return ldexpf(1.f, shift);
}
// SMP_LOG2E exactly at temperature 1; finite for a denormal temperature too (0 * c must stay 0 for the maximum's weight)
static inline float smp_host_ctau(float temperature) { return (float)fmin(1.4426950408889634 / (double)temperature, 3.4e38); }
