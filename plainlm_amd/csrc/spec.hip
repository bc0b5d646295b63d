// Speculative-sampling acceptance on the device for gfx950: k drafted tokens per sequence are checked against the
// target's k + 1 chunk rows by the rule of Leviathan et al. / Chen et al. (2023), nothing is read back and there is no workspace.
//
// p (target) and q (draft) are the distributions plm_sample_logits_bf16 draws from: its kept set is {finite x >= cutoff}, so one cutoff
// per row replaces all top-k / top-p logic here, and a weight is sample_common.h's smp_fix of the same key, maximum, c and scale - the
// very integer the draft token was drawn with.  Every sum is an integer (64-bit fixed point), so no result depends on the shape of a
// reduction; the two quotients the rule needs (alpha, and p_i - q_i of the residual) are fp64 expressions of those integers, evaluated
// the same way by whichever thread needs them.
//
// A pass over one row of 50,280 logits that takes an exponential costs a workgroup about 10 us (section 13), and a sequence has 2k + 1
// rows, so the rows must not queue behind one another on one CU.  Whether row r is accepted depends on row r alone:
//   launch 1  one workgroup per (sequence, drafted row): alpha and the verdict; logp[b, r] takes the token's log-probability, or
//             SPV_REJECTED (a log-probability is never positive) - the k + 1 output slots are the only memory between the launches;
//   launch 2  one workgroup per sequence: the first rejected row a (or k), its residual draw or the target's own token, the outputs.
// Launch 2 computes row a's sums again instead of fetching them from a workspace: two rows, whatever k is.
#include <cmath>

#include "plm_device.h"
#include "sample_common.h"

#include "../../include/plainlm_hip.h"

#define SPV_REJECTED 1.f
#define SPV_MAX_DRAFT 31  // a chunk of k + 1 <= 32 rows is one wave's queries in attn_extend_kernel

struct SpvRow {
  unsigned kmax;  // key of the largest finite logit, 0 when the row has none
  float xmax;
  smp_u64 Z;      // sum of the kept weights at the launch's temperature
  smp_u64 S1;     // sum of every finite logit's weight at temperature 1 (the partition sum of logp)
};

// f(bf16 bits) for every column this thread owns in one block-wide pass over row[0, V): 16-byte loads between a peeled head and tail,
// as sample_kernel's pass A reads a row; no column >= V is touched
template <class F>
__device__ __forceinline__ void spv_for_cols(const uint16_t* __restrict__ row, int V, F f) {
  const int tid = threadIdx.x;
  const int head = min(V, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 1));
  const int nvec = (V - head) >> 3;
  if (tid < head) f((unsigned)row[tid]);
  for (int v = tid; v < nvec; v += SMP_THREADS) {
    const u32x4_t w = *reinterpret_cast<const u32x4_t*>(row + head + 8 * (int64_t)v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f(w[j] & 0xFFFFu);
      f(w[j] >> 16);
    }
  }
  const int64_t t = (int64_t)head + 8 * (int64_t)nvec + tid;
  if (t < V) f((unsigned)row[t]);
}

// the weight sample_kernel gives a column: 0 outside the kept set {finite x >= cutoff} (a NaN cutoff keeps nothing)
__device__ __forceinline__ smp_u64 spv_weight(unsigned bits, float xmax, float cutoff, float c_tau, float scale) {
  const unsigned k = smp_key(bits);
  if (k == 0u) return 0ull;
  const float v = smp_value(k);
  return v >= cutoff ? smp_fix(v - xmax, c_tau, scale) : 0ull;
}

// Two passes over one row by the whole block (the second one L2-hot): the maximum, then the sums.  Every thread receives the result.
template <bool WANT_S1>
__device__ __forceinline__ SpvRow spv_row_stats(const uint16_t* __restrict__ row, int V, float cutoff, float c_tau, float scale,
                                                smp_u64* s_part) {
  unsigned kmax = 0;
  spv_for_cols(row, V, [&](unsigned bits) { kmax = max(kmax, smp_key(bits)); });
  SpvRow st;
  st.kmax = (unsigned)smp_block_max(kmax, s_part);
  st.xmax = smp_value(st.kmax);
  st.Z = st.S1 = 0ull;
  if (st.kmax == 0u) return st;  // the whole block: no finite logit
  const float xmax = st.xmax;
  smp_u64 z = 0, s1 = 0;
  spv_for_cols(row, V, [&](unsigned bits) {
    const unsigned k = smp_key(bits);
    if (k == 0u) return;
    const float v = smp_value(k), d = v - xmax;
    if (v >= cutoff) z += smp_fix(d, c_tau, scale);
    if (WANT_S1) s1 += smp_fix(d, SMP_LOG2E, scale);
  });
  st.Z = smp_block_sum(z, s_part);
  if (WANT_S1) st.S1 = smp_block_sum(s1, s_part);
  return st;
}

// log softmax over all V raw logits at temperature 1, as sample_kernel states it; NaN for a non-finite logit
__device__ __forceinline__ float spv_logp(unsigned bits, const SpvRow& st, float scale) {
  const unsigned k = smp_key(bits);
  if (k == 0u || st.kmax == 0u) return __uint_as_float(0x7FC00000u);
  return (smp_value(k) - st.xmax) - logf((float)((double)st.S1 / (double)scale));
}

__device__ __forceinline__ float spv_clamp_u(float u) {
  u = u >= 0.f ? u : 0.f;  // NaN and negative values
  return u < 1.f ? u : __uint_as_float(0x3F7FFFFFu);
}

// ---- launch 1: block r + k * b decides drafted row r of sequence b ------------------------------------------------------------------
__global__ __launch_bounds__(SMP_THREADS) void spec_rows_kernel(const uint16_t* __restrict__ p, int64_t ldp, const uint16_t* __restrict__ q,
                                                                int64_t ldq, const int64_t* __restrict__ draft_tok,
                                                                const float* __restrict__ p_cutoff, const float* __restrict__ q_cutoff,
                                                                const float* __restrict__ u_acc, float c_tau, float scale,
                                                                float* __restrict__ logp, int64_t B, int k, int V) {
  __shared__ smp_u64 s_part[SMP_WAVES];
  const int64_t b = blockIdx.x / k;
  const int r = (int)(blockIdx.x - b * k);
  const int64_t pr = b * (k + 1) + r, qr = (int64_t)r * B + b;
  const uint16_t* prow = p + pr * ldp;
  const uint16_t* qrow = q + qr * ldq;
  const float cp = p_cutoff[pr], cq = q_cutoff[qr];
  const int64_t x = draft_tok[qr];
  float* slot = logp + pr;

  // alpha = 0 without a pass over either row: a token outside [0, V) or outside p's kept set (the same for every thread)
  unsigned xbits = 0, xk = 0;
  bool accept = x >= 0 && x < V;
  if (accept) {
    xbits = prow[x];
    xk = smp_key(xbits);
    accept = xk != 0u && smp_value(xk) >= cp;
  }
  if (!accept) {
    if (threadIdx.x == 0) *slot = SPV_REJECTED;
    return;
  }
  const SpvRow P = spv_row_stats<true>(prow, V, cp, c_tau, scale, s_part);
  const smp_u64 wp = smp_fix(smp_value(xk) - P.xmax, c_tau, scale);
  accept = wp != 0ull;  // p(x) rounds to 0: alpha = 0
  const unsigned qk = smp_key(qrow[x]);
  if (accept && qk != 0u && smp_value(qk) >= cq) {  // else q(x) = 0 < p(x): alpha = 1
    const SpvRow Q = spv_row_stats<false>(qrow, V, cq, c_tau, scale, s_part);
    const smp_u64 wq = smp_fix(smp_value(qk) - Q.xmax, c_tau, scale);
    if (wq != 0ull) {
      const double alpha = ((double)wp * (double)Q.Z) / ((double)wq * (double)P.Z);  // p(x) / q(x); P.Z >= wp > 0
      accept = (double)spv_clamp_u(u_acc[qr]) < alpha;
    }
  }
  if (threadIdx.x == 0) *slot = accept ? spv_logp(xbits, P, scale) : SPV_REJECTED;
}

// ---- launch 2: block b finishes sequence b ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SMP_THREADS) void spec_finish_kernel(const uint16_t* __restrict__ p, int64_t ldp, const uint16_t* __restrict__ q,
                                                                  int64_t ldq, const float* __restrict__ p_cutoff,
                                                                  const float* __restrict__ q_cutoff, const int64_t* __restrict__ p_tok,
                                                                  const float* __restrict__ u_res, float c_tau, float scale,
                                                                  int32_t* __restrict__ n_accept, int64_t* __restrict__ next_tok,
                                                                  float* logp, int64_t B, int k, int V) {
  __shared__ smp_u64 s_part[SMP_WAVES];
  __shared__ smp_u64 s_res;
  const int tid = threadIdx.x, lane = tid % PLM_WAVE, wave = tid / PLM_WAVE;
  const int64_t b = blockIdx.x;
  int a = k;  // the first rejected row; every thread reads the same slots, thread 0 writes them only after the barriers below
  for (int r = k - 1; r >= 0; --r)
    if (logp[b * (k + 1) + r] > 0.f) a = r;
  const int64_t pr = b * (k + 1) + a;
  const uint16_t* prow = p + pr * ldp;
  const float cp = p_cutoff[pr];
  const SpvRow P = spv_row_stats<true>(prow, V, cp, c_tau, scale, s_part);
  int64_t tok = p_tok[pr];  // the bonus token (a = k), and what a row without a residual falls back to
  tok = tok < 0 ? 0 : (tok >= V ? (int64_t)V - 1 : tok);

  if (a < k && P.Z != 0ull) {  // the same for the whole block
    const int64_t qr = (int64_t)a * B + b;
    const uint16_t* qrow = q + qr * ldq;
    const float cq = q_cutoff[qr];
    const SpvRow Q = spv_row_stats<false>(qrow, V, cq, c_tau, scale, s_part);
    const double inv_zp = 1.0 / (double)P.Z, inv_zq = Q.Z != 0ull ? 1.0 / (double)Q.Z : 0.0, dscale = (double)scale;
    // max(0, p_i - q_i) as fixed point: at most `scale`, so a sum of V of them stays below 2^63 like the weights'
    auto residual = [&](int64_t i) -> smp_u64 {
      const smp_u64 wp = spv_weight(prow[i], P.xmax, cp, c_tau, scale);
      if (wp == 0ull) return 0ull;
      const smp_u64 wq = spv_weight(qrow[i], Q.xmax, cq, c_tau, scale);
      const double d = (double)wp * inv_zp - (double)wq * inv_zq;
      return d > 0.0 ? (smp_u64)(d * dscale) : 0ull;
    };
    // wave w owns the columns [w * seg, (w + 1) * seg), its lanes stride through them: coalesced loads, and the running sum in
    // ascending column order is (the waves before) + (the 64-column groups before) + (a scan over the lanes)
    const int64_t seg = ((int64_t)V + SMP_WAVES - 1) / SMP_WAVES;
    const int64_t c0 = min((int64_t)V, wave * seg), c1 = min((int64_t)V, c0 + seg);
    smp_u64 mine = 0;
    for (int64_t i = c0 + lane; i < c1; i += PLM_WAVE) mine += residual(i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, PLM_WAVE);
    if (lane == 0) s_part[wave] = mine;
    if (tid == 0) s_res = SMP_NONE;
    __syncthreads();
    smp_u64 R = 0, base = 0;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; ++w) {
      const smp_u64 t = s_part[w];
      base += w < wave ? t : 0ull;
      R += t;
    }
    const smp_u64 T = (smp_u64)((double)spv_clamp_u(u_res[b]) * (double)R);  // floor(u R) < R: for integers C, C > u R is C > floor(u R)
    if (base <= T && T < base + mine) {  // one wave at most (none when R = 0)
      smp_u64 acc = base;
      for (int64_t i0 = c0; i0 < c1; i0 += PLM_WAVE) {
        const int64_t i = i0 + lane;
        smp_u64 v = i < c1 ? residual(i) : 0ull;
#pragma unroll
        for (int o = 1; o < PLM_WAVE; o <<= 1) {
          const smp_u64 t = __shfl_up(v, o, PLM_WAVE);
          if (lane >= o) v += t;
        }
        const unsigned long long crossed = __ballot(acc + v > T);
        if (crossed != 0ull) {
          if (lane == __ffsll(crossed) - 1) s_res = (smp_u64)i;
          break;
        }
        acc += __shfl(v, PLM_WAVE - 1, PLM_WAVE);
      }
    }
    __syncthreads();
    if (s_res != SMP_NONE) tok = (int64_t)s_res;
  }
  if (tid == 0) {
    n_accept[b] = a;
    next_tok[b] = tok;
    logp[pr] = spv_logp(prow[tok], P, scale);
    for (int j = a + 1; j <= k; ++j) logp[b * (k + 1) + j] = 0.f;
  }
}

extern "C" int plm_spec_verify_bf16(const uint16_t* p_logits, int64_t ldp, const uint16_t* q_logits, int64_t ldq, const int64_t* draft_tok,
                                    const float* p_cutoff, const float* q_cutoff, const int64_t* p_tok, const float* u_accept,
                                    const float* u_resid, float temperature, int32_t* n_accept, int64_t* next_tok, float* logp, int64_t B,
                                    int64_t k, int64_t V, void* stream) {
  PLM_REQUIRE(p_logits && q_logits && draft_tok && p_cutoff && q_cutoff && p_tok && u_accept && u_resid && n_accept && next_tok && logp,
              "plm_spec_verify_bf16: null pointer");
  PLM_REQUIRE(k >= 1 && k <= SPV_MAX_DRAFT, "plm_spec_verify_bf16: k=%ld drafted tokens (need 1 <= k <= %d)", (long)k, SPV_MAX_DRAFT);
  PLM_REQUIRE(B >= 1 && B < ((int64_t)1 << 26) && V >= 1 && V < ((int64_t)1 << 31) && ldp >= V && ldq >= V,
              "plm_spec_verify_bf16: bad shape B=%ld V=%ld ldp=%ld ldq=%ld (need 1 <= B < 2^26, 1 <= V < 2^31 and ld >= V)", (long)B, (long)V,
              (long)ldp, (long)ldq);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(p_logits) | reinterpret_cast<uintptr_t>(q_logits)) & 1) == 0,
              "plm_spec_verify_bf16: logits must be 2-byte aligned");
  PLM_REQUIRE(std::isfinite(temperature) && temperature > 0.f, "plm_spec_verify_bf16: temperature %g must be finite and > 0",
              (double)temperature);
  const float scale = smp_host_scale(V), c_tau = smp_host_ctau(temperature);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(spec_rows_kernel, dim3((unsigned)(B * k)), dim3(SMP_THREADS), 0, s, p_logits, ldp, q_logits, ldq, draft_tok, p_cutoff,
                     q_cutoff, u_accept, c_tau, scale, logp, B, (int)k, (int)V);
  PLM_CHECK_LAUNCH("plm_spec_verify_bf16");
  hipLaunchKernelGGL(spec_finish_kernel, dim3((unsigned)B), dim3(SMP_THREADS), 0, s, p_logits, ldp, q_logits, ldq, p_cutoff, q_cutoff, p_tok,
                     u_resid, c_tau, scale, n_accept, next_tok, logp, B, (int)k, (int)V);
  PLM_CHECK_LAUNCH("plm_spec_verify_bf16");
  return PLM_OK;
}

// ---- one-hot acceptance: the draft is a deterministic proposal (plm_lookup_draft_i64) ----------------------------
// q is one-hot on the proposed token x, so alpha = p(x) and the residual is p with x removed.  In the sampler's fixed point both are
// integers: u < w_x / Z is floor(u Z) < w_x (w_x is an integer), the test the sampler's own draw makes of a running sum; the residual
// weight of a column is the column's own weight, R = Z - w_x, and the draw is the sampler's walk with column x's weight set to 0.  No
// quotient of two distributions is left.  The launches have plm_spec_verify_bf16's shape; rows at and beyond n_prop[b] are never loaded.
__device__ __forceinline__ int spl_n_prop(const int32_t* __restrict__ n_prop, int64_t b, int k) {
  const int n = n_prop[b];
  return n < 0 ? 0 : (n > k ? k : n);
}

// launch 1: block r + k * b decides proposed row r of sequence b; a row at or beyond n_prop[b] leaves its slot alone (launch 2 reads none)
__global__ __launch_bounds__(SMP_THREADS) void spec_lookup_rows_kernel(const uint16_t* __restrict__ p, int64_t ldp,
                                                                       const int64_t* __restrict__ draft_tok, const int32_t* __restrict__ n_prop,
                                                                       const float* __restrict__ p_cutoff, const float* __restrict__ u_acc,
                                                                       float c_tau, float scale, float* __restrict__ logp, int64_t B, int k,
                                                                       int V) {
  __shared__ smp_u64 s_part[SMP_WAVES];
  const int64_t b = blockIdx.x / k;
  const int r = (int)(blockIdx.x - b * k);
  if (r >= spl_n_prop(n_prop, b, k)) return;  // the whole block
  const int64_t pr = b * (k + 1) + r;
  const uint16_t* prow = p + pr * ldp;
  const float cp = p_cutoff[pr];
  const int64_t x = draft_tok[b * k + r];
  float* slot = logp + pr;

  // alpha = 0 without a pass over the row: a token outside [0, V) or outside p's kept set (the same for every thread)
  unsigned xbits = 0, xk = 0;
  bool accept = x >= 0 && x < V;
  if (accept) {
    xbits = prow[x];
    xk = smp_key(xbits);
    accept = xk != 0u && smp_value(xk) >= cp;
  }
  if (!accept) {
    if (threadIdx.x == 0) *slot = SPV_REJECTED;
    return;
  }
  const SpvRow P = spv_row_stats<true>(prow, V, cp, c_tau, scale, s_part);
  const smp_u64 wx = smp_fix(smp_value(xk) - P.xmax, c_tau, scale);  // 0: p(x) rounds to 0, alpha = 0
  accept = (smp_u64)((double)spv_clamp_u(u_acc[(int64_t)r * B + b]) * (double)P.Z) < wx;  // floor(u Z) < w_x; u < 1, so the product is < 2^63
  if (threadIdx.x == 0) *slot = accept ? spv_logp(xbits, P, scale) : SPV_REJECTED;
}

// launch 2: block b finishes sequence b
__global__ __launch_bounds__(SMP_THREADS) void spec_lookup_finish_kernel(const uint16_t* __restrict__ p, int64_t ldp,
                                                                         const int64_t* __restrict__ draft_tok,
                                                                         const int32_t* __restrict__ n_prop, const float* __restrict__ p_cutoff,
                                                                         const int64_t* __restrict__ p_tok, const float* __restrict__ u_res,
                                                                         float c_tau, float scale, int32_t* __restrict__ n_accept,
                                                                         int64_t* __restrict__ next_tok, float* logp, int k, int V) {
  __shared__ smp_u64 s_part[SMP_WAVES];
  __shared__ smp_u64 s_res;
  const int tid = threadIdx.x, lane = tid % PLM_WAVE, wave = tid / PLM_WAVE;
  const int64_t b = blockIdx.x;
  const int np = spl_n_prop(n_prop, b, k);
  int a = np;  // the first rejected row; every thread reads the same slots, thread 0 writes them only after the barriers below
  for (int r = np - 1; r >= 0; --r)
    if (logp[b * (k + 1) + r] > 0.f) a = r;
  const int64_t pr = b * (k + 1) + a;
  const uint16_t* prow = p + pr * ldp;
  const float cp = p_cutoff[pr];
  const SpvRow P = spv_row_stats<true>(prow, V, cp, c_tau, scale, s_part);
  int64_t tok = p_tok[pr];  // the bonus token (a = n_prop), and what a row without a residual falls back to
  tok = tok < 0 ? 0 : (tok >= V ? (int64_t)V - 1 : tok);

  if (a < np && P.Z != 0ull) {  // the same for the whole block
    const int64_t x = draft_tok[b * k + a];
    auto residual = [&](int64_t i) -> smp_u64 { return i == x ? 0ull : spv_weight(prow[i], P.xmax, cp, c_tau, scale); };
    // spec_finish_kernel's walk: wave w owns the columns [w * seg, (w + 1) * seg), its lanes stride through them
    const int64_t seg = ((int64_t)V + SMP_WAVES - 1) / SMP_WAVES;
    const int64_t c0 = min((int64_t)V, wave * seg), c1 = min((int64_t)V, c0 + seg);
    smp_u64 mine = 0;
    for (int64_t i = c0 + lane; i < c1; i += PLM_WAVE) mine += residual(i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, PLM_WAVE);
    if (lane == 0) s_part[wave] = mine;
    if (tid == 0) s_res = SMP_NONE;
    __syncthreads();
    smp_u64 R = 0, base = 0;  // R = Z - w_x
#pragma unroll
    for (int w = 0; w < SMP_WAVES; ++w) {
      const smp_u64 t = s_part[w];
      base += w < wave ? t : 0ull;
      R += t;
    }
    const smp_u64 T = (smp_u64)((double)spv_clamp_u(u_res[b]) * (double)R);  // floor(u R) < R
    if (base <= T && T < base + mine) {  // one wave at most (none when R = 0)
      smp_u64 acc = base;
      for (int64_t i0 = c0; i0 < c1; i0 += PLM_WAVE) {
        const int64_t i = i0 + lane;
        smp_u64 v = i < c1 ? residual(i) : 0ull;
#pragma unroll
        for (int o = 1; o < PLM_WAVE; o <<= 1) {
          const smp_u64 t = __shfl_up(v, o, PLM_WAVE);
          if (lane >= o) v += t;
        }
        const unsigned long long crossed = __ballot(acc + v > T);
        if (crossed != 0ull) {
          if (lane == __ffsll(crossed) - 1) s_res = (smp_u64)i;
          break;
        }
        acc += __shfl(v, PLM_WAVE - 1, PLM_WAVE);
      }
    }
    __syncthreads();
    if (s_res != SMP_NONE) tok = (int64_t)s_res;
  }
  if (tid == 0) {
    n_accept[b] = a;
    next_tok[b] = tok;
    logp[pr] = spv_logp(prow[tok], P, scale);
    for (int j = a + 1; j <= k; ++j) logp[b * (k + 1) + j] = 0.f;
  }
}

extern "C" int plm_spec_verify_lookup_bf16(const uint16_t* p_logits, int64_t ldp, const int64_t* draft_tok, const int32_t* n_prop,
                                           const float* p_cutoff, const int64_t* p_tok, const float* u_accept, const float* u_resid,
                                           float temperature, int32_t* n_accept, int64_t* next_tok, float* logp, int64_t B, int64_t k,
                                           int64_t V, void* stream) {
  PLM_REQUIRE(p_logits && draft_tok && n_prop && p_cutoff && p_tok && u_accept && u_resid && n_accept && next_tok && logp,
              "plm_spec_verify_lookup_bf16: null pointer");
  PLM_REQUIRE(k >= 1 && k <= SPV_MAX_DRAFT, "plm_spec_verify_lookup_bf16: k=%ld drafted tokens (need 1 <= k <= %d)", (long)k, SPV_MAX_DRAFT);
  PLM_REQUIRE(B >= 1 && B < ((int64_t)1 << 26) && V >= 1 && V < ((int64_t)1 << 31) && ldp >= V,
              "plm_spec_verify_lookup_bf16: bad shape B=%ld V=%ld ldp=%ld (need 1 <= B < 2^26, 1 <= V < 2^31 and ldp >= V)", (long)B, (long)V,
              (long)ldp);
  PLM_REQUIRE((reinterpret_cast<uintptr_t>(p_logits) & 1) == 0, "plm_spec_verify_lookup_bf16: logits must be 2-byte aligned");
  PLM_REQUIRE(std::isfinite(temperature) && temperature > 0.f, "plm_spec_verify_lookup_bf16: temperature %g must be finite and > 0",
              (double)temperature);
  const float scale = smp_host_scale(V), c_tau = smp_host_ctau(temperature);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(spec_lookup_rows_kernel, dim3((unsigned)(B * k)), dim3(SMP_THREADS), 0, s, p_logits, ldp, draft_tok, n_prop, p_cutoff,
                     u_accept, c_tau, scale, logp, B, (int)k, (int)V);
  PLM_CHECK_LAUNCH("plm_spec_verify_lookup_bf16");
  hipLaunchKernelGGL(spec_lookup_finish_kernel, dim3((unsigned)B), dim3(SMP_THREADS), 0, s, p_logits, ldp, draft_tok, n_prop, p_cutoff, p_tok,
                     u_resid, c_tau, scale, n_accept, next_tok, logp, (int)k, (int)V);
  PLM_CHECK_LAUNCH("plm_spec_verify_lookup_bf16");
  return PLM_OK;
}
