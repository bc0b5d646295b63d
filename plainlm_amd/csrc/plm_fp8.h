// OCP e4m3fn elements under E8M0 power-of-two block scales: the arithmetic shared by the MXFP8 operands (mx.hip, blocks of 32, DESIGN.md
// section 9) and the FP8 KV cache (attn_cache.hip, decode_fused.hip, blocks of 16).  gfx950's FP8 is OCP, not fnuz.
//
// Scale rule (exact, shared with the CPU references tests/mx_ref.py and tests/kv8_ref.py): amax = max |x| of the block, E = floor(log2 amax),
// e = E - 8 if amax <= 448 * 2^(E-8) (= 1.75 * 2^E) else E - 7 - the smallest e with amax <= 448 * 2^e -, clamped to [-127, 127]; scale
// byte e + 127; q = RNE_e4m3fn(x * 2^-e) with subnormals.  amax = 0: scale byte 0, zero elements.  Any non-finite element: scale byte 0xFF
// and every element 0x7F (NaN).
#pragma once
#include "plm_device.h"

// RNE to e4m3fn of a finite |y| <= 448 (by construction of the scale): code = sign | exponent(4) | mantissa(3), bias 7, subnormal step 2^-9
__device__ __forceinline__ unsigned mx_e4m3(float y) {
  const unsigned u = __float_as_uint(y);
  const unsigned sgn = (u >> 24) & 0x80u;
  const float a = __builtin_fabsf(y);
  const unsigned sub = (unsigned)__builtin_rintf(a * 512.f);  // |y| < 2^-6: multiples of 2^-9, v_rndne_f32 is RNE (8 = the smallest normal)
  unsigned b = __float_as_uint(a);
  b += 0x7FFFFu + ((b >> 20) & 1u);                             // RNE to 3 mantissa bits
  const unsigned nrm = (b >> 20) - (120u << 3);                  // rebias 127 -> 7
  return sgn | (a < 0.015625f ? sub : nrm);
}

// e of the scale rule for a finite amax > 0 (an fp32 holding a bf16 value, subnormals included)
__device__ __forceinline__ int mx_scale_exp(float amax) {
  const unsigned ab = __float_as_uint(amax);
  const unsigned ex = ab >> 23;
  int E, over;
  if (ex != 0) {
    E = (int)ex - 127;
    over = (ab & 0x7FFFFFu) > 0x600000u;
  } else {  // fp32 (= bf16) subnormal: amax = m * 2^-149
    const int p = 31 - __builtin_clz(ab);
    E = p - 149;
    over = ab > (7u << (p - 2));
  }
  int e = E - 8 + over;
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// ---- the FP8 KV cache's 16-element blocks ----------------------------------------------------------------------------------------
// |x| for the block maximum, +inf for a non-finite x (fmaxf would drop a NaN): amax == +inf marks a block that holds one
__device__ __forceinline__ float kv8_mag(float x) {
  return (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u ? INFINITY : __builtin_fabsf(x);
}

// the scale byte of a block whose kv8_mag maximum is amax
__device__ __forceinline__ unsigned kv8_scale_byte(float amax) {
  if (amax == INFINITY) return 0xFFu;
  if (amax == 0.f) return 0u;
  return (unsigned)(mx_scale_exp(amax) + 127);
}

// the code of element x of that block (sb = kv8_scale_byte(amax))
__device__ __forceinline__ unsigned kv8_code(float x, float amax, unsigned sb) {
  if (amax == INFINITY) return 0x7Fu;
  if (amax == 0.f) return 0u;  // not the sign bit of a -0
  return mx_e4m3(__builtin_ldexpf(x, 127 - (int)sb));
}

// 2^(s - 127) of a scale byte, NaN for 0xFF.  s = 0 is 2^-127, an fp32 subnormal: the kernels run with fp32 subnormals kept (hipcc's
// default mode), so code * kv8_scale(s) is exact in fp32 down to 2^-149 and, rounded to bf16, exact down to bf16's smallest subnormal
// 2^-133; a value below that (a block whose amax is under 2^-124) rounds, and nothing the model computes lives there.
__device__ __forceinline__ float kv8_scale(unsigned s) {
  return __uint_as_float(s == 0u ? 0x00400000u : (s == 0xFFu ? 0x7FC00000u : s << 23));
}

// four / eight codes (byte j of the dword = element j) times the block's scale.  v_cvt_pk_f32_fp8 is the OCP e4m3fn conversion on gfx950
// (0x7F / 0xFF are NaN); the product with a power of two is exact.
__device__ __forceinline__ void kv8_deq4(unsigned w, float f, float* o) {
  typedef __attribute__((ext_vector_type(2))) float f32x2_t;
  const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  o[0] = lo[0] * f;
  o[1] = lo[1] * f;
  o[2] = hi[0] * f;
  o[3] = hi[1] * f;
}

__device__ __forceinline__ void kv8_deq8(u32x2_t w, unsigned s, float (&o)[8]) {
  const float f = kv8_scale(s);
  kv8_deq4(w[0], f, o);
  kv8_deq4(w[1], f, o + 4);
}

__device__ __forceinline__ bf16x8_t kv8_deq8_bf16(u32x2_t w, unsigned s) {
  float o[8];
  kv8_deq8(w, s, o);
  bf16x8_t r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = f2bf(o[e]);
  return r;
}

// One block of 16 values: 4 packed dwords (element j in byte j & 3 of dword j >> 2) and the scale byte.
__device__ __forceinline__ unsigned kv8_block(const float (&v)[16], u32x4_t& q) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) amax = __builtin_fmaxf(amax, kv8_mag(v[j]));
  const unsigned sb = kv8_scale_byte(amax);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned w = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) w |= kv8_code(v[4 * j + i], amax, sb) << (8 * i);
    q[j] = w;
  }
  return sb;
}

// bytes of a cache row's payload: k codes dm | v codes dm | k scales dm/16 | v scales dm/16
__host__ __device__ __forceinline__ int64_t kv8_row_payload(int64_t dm) { return 2 * dm + dm / 8; }
