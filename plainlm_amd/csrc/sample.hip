// On-device sampling for gfx950: temperature, top-k by value, top-p by value class and the draw, one token per row
// of bf16 logits, in one launch with one workgroup per row and no workspace.
//
// bf16 gives a 16-bit order-preserving key (smp_key; -0 is folded into +0 so that equal VALUES have equal keys, non-finite logits get
// key 0).  The row is read from global memory once and kept in LDS as keys (65,536 columns = 128 KiB of the CU's 160 KiB; wider rows
// re-read global memory, L2-hot, through the same code).  Both thresholds come from two histogram levels over the key - 2,048 bins of
// key >> 5 (sign, exponent and three mantissa bits: few lanes of a wave meet in one bin), then the 32 keys of the one bin that holds the
// threshold.  Every sum is an integer: counts, and weights as 64-bit fixed point (w * 2^40 with w <= 1; the host lowers the shift until
// V * 2^shift < 2^63).  Integer adds commute, so neither the LDS atomics' arrival order nor the shape of a reduction can change a
// bit of any result, and the draw's running sums C_i are exact sums of the rounded weights: a thread owns a contiguous chunk of columns,
// a block-wide scan of the chunk sums finds the chunk that crosses u * Z, its owner walks it again.
#include <cmath>

#include "plm_device.h"
#include "sample_common.h"

#include "../../include/plainlm_hip.h"

#define SMP_LDS_COLS 65536   // columns of a row kept in LDS
#define SMP_BINS1 2048       // level 1: key >> 5
#define SMP_BINS2 32         // level 2: key & 31, inside one level-1 bin
static_assert(SMP_BINS1 == 2 * SMP_THREADS, "smp_find1: two level-1 bins per thread");

// Level 1: the highest bin b with hist[b] + hist[b + 1] + ... >= target (target >= 1), and `above` = the sum over the bins beyond b.
// False when the whole histogram holds less than target.
template <class T>
__device__ __forceinline__ bool smp_find1(const T* hist, smp_u64 target, smp_u64* s_part, smp_u64* s_res, unsigned& bin, smp_u64& above) {
  const int hi = SMP_BINS1 - 1 - 2 * (int)threadIdx.x;  // descending: thread t owns bins hi, hi - 1
  const smp_u64 vh = hist[hi], vl = hist[hi - 1];
  if (threadIdx.x == 0) s_res[0] = SMP_NONE;
  smp_u64 total;
  const smp_u64 incl = smp_block_scan(vh + vl, s_part, total);
  const smp_u64 excl = incl - (vh + vl);
  if (excl < target && incl >= target) {  // one thread at most: the running sum does not decrease
    const bool in_hi = excl + vh >= target;
    s_res[0] = in_hi ? hi : hi - 1;
    s_res[1] = in_hi ? excl : excl + vh;
  }
  __syncthreads();
  const smp_u64 r = s_res[0];
  above = s_res[1];
  __syncthreads();
  bin = (unsigned)r;
  return r != SMP_NONE;
}

template <bool CACHED>
__global__ __launch_bounds__(SMP_THREADS) void sample_kernel(const uint16_t* __restrict__ logits, int64_t ld, const float* __restrict__ u,
                                                             float c_tau, int top_k, float top_p, float scale, int64_t* __restrict__ tok,
                                                             float* __restrict__ logp, int32_t* __restrict__ n_kept,
                                                             float* __restrict__ cutoff, int V) {
  __shared__ uint16_t s_key[CACHED ? SMP_LDS_COLS : 8];
  __shared__ unsigned s_cnt1[SMP_BINS1];
  __shared__ smp_u64 s_mass1[SMP_BINS1];
  __shared__ unsigned s_cnt2[SMP_BINS2];
  __shared__ smp_u64 s_mass2[SMP_BINS2];
  __shared__ smp_u64 s_part[SMP_WAVES];
  __shared__ smp_u64 s_res[2];

  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const uint16_t* row = logits + b * ld;
  auto key = [&](int64_t i) -> unsigned { return CACHED ? (unsigned)s_key[i] : smp_key(row[i]); };

  // ---- pass A: the one read of the row (16-byte loads between a peeled head and tail; no column >= V is touched), keys into LDS,
  // the maximum.  The histograms are cleared under the same barriers.
  unsigned kmax = 0;
  if (CACHED) {
    const int head = min(V, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(row) & 15u)) & 15u) >> 1));
    const int nvec = (V - head) >> 3;
    if (tid < head) {
      const unsigned k = smp_key(row[tid]);
      s_key[tid] = (uint16_t)k;
      kmax = k;
    }
    for (int v = tid; v < nvec; v += SMP_THREADS) {
      const int c = head + 8 * v;
      const u32x4_t q = *reinterpret_cast<const u32x4_t*>(row + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned k0 = smp_key(q[j] & 0xFFFFu), k1 = smp_key(q[j] >> 16);
        s_key[c + 2 * j] = (uint16_t)k0;
        s_key[c + 2 * j + 1] = (uint16_t)k1;
        kmax = max(kmax, max(k0, k1));
      }
    }
    const int t = head + 8 * nvec + tid;
    if (t < V) {
      const unsigned k = smp_key(row[t]);
      s_key[t] = (uint16_t)k;
      kmax = max(kmax, k);
    }
  } else {
    for (int64_t i = tid; i < V; i += SMP_THREADS) kmax = max(kmax, smp_key(row[i]));
  }
  for (int i = tid; i < SMP_BINS1; i += SMP_THREADS) {
    s_cnt1[i] = 0u;
    s_mass1[i] = 0ull;
  }
  if (tid < SMP_BINS2) {
    s_cnt2[tid] = 0u;
    s_mass2[tid] = 0ull;
  }
  kmax = (unsigned)smp_block_max(kmax, s_part);
  if (kmax == 0u) {  // no finite logit in the row
    if (tid == 0) {
      tok[b] = 0;
      logp[b] = __uint_as_float(0x7FC00000u);
      if (n_kept != nullptr) n_kept[b] = 0;
      if (cutoff != nullptr) cutoff[b] = __uint_as_float(0x7FC00000u);
    }
    return;
  }
  const float xmax = smp_value(kmax);

  // ---- pass B: level-1 counts and masses of every finite logit, and the temperature-1 partition sum for logp
  // (a filter that is off does not pay for its histogram: top_k = 0 never reads the counts, top_p = 1 never reads the masses)
  smp_u64 s1 = 0;
  for (int64_t i = tid; i < V; i += SMP_THREADS) {
    const unsigned k = key(i);
    if (k == 0u) continue;
    const float d = smp_value(k) - xmax;
    if (top_k > 0) atomicAdd(&s_cnt1[k >> 5], 1u);
    if (top_p < 1.f || c_tau == SMP_LOG2E) {
      const smp_u64 w = smp_fix(d, c_tau, scale);
      if (top_p < 1.f && w != 0ull) atomicAdd(&s_mass1[k >> 5], w);
      if (c_tau == SMP_LOG2E) s1 += w;
    }
    if (c_tau != SMP_LOG2E) s1 += smp_fix(d, SMP_LOG2E, scale);
  }
  s1 = smp_block_sum(s1, s_part);  // its barriers also publish the histograms

  // level 2 of bin b1: counts and masses per key
  auto level2 = [&](unsigned b1) {
    for (int64_t i = tid; i < V; i += SMP_THREADS) {
      const unsigned k = key(i);
      if ((k >> 5) != b1) continue;  // b1 >= 4: a key of 0 is never in it
      const smp_u64 w = smp_fix(smp_value(k) - xmax, c_tau, scale);
      atomicAdd(&s_cnt2[k & 31u], 1u);
      if (w != 0ull) atomicAdd(&s_mass2[k & 31u], w);
    }
    __syncthreads();
  };

  // ---- top-k: the key of the k-th largest value (every finite logit when there are fewer than k, or top-k is off)
  unsigned key_k = SMP_KEY_LO;
  unsigned b1k;
  smp_u64 above;
  if (top_k > 0 && smp_find1(s_cnt1, (smp_u64)top_k, s_part, s_res, b1k, above)) {
    level2(b1k);
    if (tid == 0) {
      smp_u64 acc = above;
      int j = SMP_BINS2 - 1;
      for (; j > 0; --j) {
        acc += s_cnt2[j];
        if (acc >= (smp_u64)top_k) break;
      }
      s_res[0] = (b1k << 5) | (unsigned)j;
    }
    __syncthreads();
    key_k = (unsigned)s_res[0];
    __syncthreads();
  }

  // ---- top-p: the largest key present whose class and everything above it hold top_p of the survivors' mass
  unsigned key_cut = key_k;
  if (top_p < 1.f) {
    smp_u64 zk = 0;
    for (int64_t i = tid; i < V; i += SMP_THREADS) {
      const unsigned k = key(i);
      if (k >= key_k) zk += smp_fix(smp_value(k) - xmax, c_tau, scale);  // key_k >= SMP_KEY_LO > 0
    }
    zk = smp_block_sum(zk, s_part);  // >= scale: the maximum survives and weighs exp(0) = 1
    smp_u64 target = (smp_u64)ceil((double)top_p * (double)zk);
    target = target < 1ull ? 1ull : (target > zk ? zk : target);
    unsigned b1p;
    if (smp_find1(s_mass1, target, s_part, s_res, b1p, above)) {  // always: the level-1 masses hold at least zk
      if (tid < SMP_BINS2) {
        s_cnt2[tid] = 0u;
        s_mass2[tid] = 0ull;
      }
      __syncthreads();
      level2(b1p);
      if (tid == 0) {
        smp_u64 acc = above;
        int j = SMP_BINS2 - 1;
        for (; j > 0; --j) {
          acc += s_mass2[j];
          if (acc >= target) break;
        }
        s_res[0] = (b1p << 5) | (unsigned)j;
      }
      __syncthreads();
      key_cut = max(key_k, (unsigned)s_res[0]);
      __syncthreads();
    }
  }

  // ---- the draw: thread t owns columns [t * chunk, (t + 1) * chunk)
  // (an odd chunk: the threads of a wave then start on different LDS banks whatever V is; the last threads may own nothing)
  const int64_t chunk = (((int64_t)V + SMP_THREADS - 1) / SMP_THREADS) | 1;
  const int64_t c0 = min((int64_t)V, tid * chunk), c1 = min((int64_t)V, c0 + chunk);
  smp_u64 wsum = 0, cnt = 0, last = 0;
  unsigned kmin_inv = 0;  // 0xFFFF - the lowest kept key
  for (int64_t i = c0; i < c1; ++i) {
    const unsigned k = key(i);
    if (k < key_cut) continue;
    const smp_u64 w = smp_fix(smp_value(k) - xmax, c_tau, scale);
    wsum += w;
    cnt += 1;
    kmin_inv = max(kmin_inv, 0xFFFFu - k);
    if (w != 0ull) last = (smp_u64)i + 1;
  }
  smp_u64 Z;
  const smp_u64 incl = smp_block_scan(wsum, s_part, Z);
  float uc = u[b];
  uc = uc >= 0.f ? uc : 0.f;  // NaN and negative values
  uc = uc < 1.f ? uc : __uint_as_float(0x3F7FFFFFu);
  const smp_u64 T = (smp_u64)((double)uc * (double)Z);  // floor(u Z) < Z: for integers C, C > u Z is C > floor(u Z)
  if (tid == 0) s_res[0] = SMP_NONE;
  __syncthreads();
  if (incl - wsum <= T && T < incl) {  // one thread: Z >= scale > T's shortfall, so the last running sum always crosses
    smp_u64 acc = incl - wsum;
    for (int64_t i = c0; i < c1; ++i) {
      const unsigned k = key(i);
      if (k < key_cut) continue;
      acc += smp_fix(smp_value(k) - xmax, c_tau, scale);
      if (acc > T) {
        s_res[0] = (smp_u64)i;
        break;
      }
    }
  }
  __syncthreads();
  smp_u64 pick = s_res[0];
  __syncthreads();
  cnt = smp_block_sum(cnt, s_part);
  kmin_inv = (unsigned)smp_block_max(kmin_inv, s_part);
  if (pick == SMP_NONE) {  // the specification's rule when no running sum crosses: the last kept column of positive weight
    last = smp_block_max(last, s_part);
    pick = last > 0 ? last - 1 : 0;
  }
  if (tid == 0) {
    tok[b] = (int64_t)pick;
    const float lse = logf((float)((double)s1 / (double)scale));  // s1 >= scale
    logp[b] = (smp_value(key((int64_t)pick)) - xmax) - lse;
    if (n_kept != nullptr) n_kept[b] = (int32_t)cnt;
    if (cutoff != nullptr) cutoff[b] = smp_value(0xFFFFu - kmin_inv);
  }
}

extern "C" int plm_sample_logits_bf16(const uint16_t* logits, int64_t ld, const float* u, float temperature, int64_t top_k, float top_p,
                                      int64_t* tok, float* logp, int32_t* n_kept, float* cutoff, int64_t B, int64_t V, void* stream) {
  PLM_REQUIRE(logits && u && tok && logp, "plm_sample_logits_bf16: null pointer");
  PLM_REQUIRE(B >= 1 && B < ((int64_t)1 << 31) && V >= 1 && V < ((int64_t)1 << 31) && ld >= V,
              "plm_sample_logits_bf16: bad shape B=%ld V=%ld ld=%ld (need 1 <= B, V < 2^31 and ld >= V)", (long)B, (long)V, (long)ld);
  PLM_REQUIRE((reinterpret_cast<uintptr_t>(logits) & 1) == 0, "plm_sample_logits_bf16: logits must be 2-byte aligned");
  PLM_REQUIRE(std::isfinite(temperature) && temperature > 0.f, "plm_sample_logits_bf16: temperature %g must be finite and > 0",
              (double)temperature);
  PLM_REQUIRE(top_k >= 0, "plm_sample_logits_bf16: top_k %ld must be >= 0 (0 = off)", (long)top_k);
  PLM_REQUIRE(top_p > 0.f && top_p <= 1.f, "plm_sample_logits_bf16: top_p %g must be in (0, 1] (1 = off)", (double)top_p);
  const float scale = smp_host_scale(V);
  const int k = top_k >= V ? 0 : (int)top_k;
  const float c_tau = smp_host_ctau(temperature);
  hipStream_t s = (hipStream_t)stream;
  if (V <= SMP_LDS_COLS)
    hipLaunchKernelGGL(sample_kernel<true>, dim3((unsigned)B), dim3(SMP_THREADS), 0, s, logits, ld, u, c_tau, k, top_p, scale, tok, logp,
                       n_kept, cutoff, (int)V);
  else
    hipLaunchKernelGGL(sample_kernel<false>, dim3((unsigned)B), dim3(SMP_THREADS), 0, s, logits, ld, u, c_tau, k, top_p, scale, tok, logp,
                       n_kept, cutoff, (int)V);
  PLM_CHECK_LAUNCH("plm_sample_logits_bf16");
  return PLM_OK;
}
