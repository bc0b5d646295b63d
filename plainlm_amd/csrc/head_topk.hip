// Head top-k for gfx950: per row of bf16 logits the k <= 64 largest columns with their log-probabilities, the row's
// log-sum-exp and the 0-based rank of a target column.  plm_head_topk_bf16 (gemm_api.hip) produces the logits a chunk of rows at a time
// into its workspace, so a row comes from L2 / the Infinity Cache; this kernel loads it from there exactly once.
//
// head_topk_rows_kernel<ROW_IN_LDS>, one 1024-thread workgroup per row:
//   stage    16-byte global loads put the row into LDS (V = 50280: 100,560 bytes of the CU's 160 KB); the same loop takes the maximum of
//            the order-preserving 16-bit keys (sample_common.h: NaN and the infinities have key 0 and are no candidates, +0 == -0) per
//            thread and per row.  Every later pass reads LDS.  ROW_IN_LDS = false (a row beyond HT_ROW_LDS_BYTES) reads global memory
//            again in every pass instead: the chunk was written a moment ago and sits in cache.
//   bound    the k-th largest of the 1024 THREAD maxima, by the radix select below over 1024 keys.  k columns at least are as large, so
//            the k-th largest column is: only keys >= this bound enter the row's histograms - a few hundred LDS atomics per row in
//            place of V of them on the handful of bins that hold a row of logits.  Fewer than k threads with a finite logit: no bound.
//   select   radix select over the 16-bit keys: a 256-bin LDS histogram of the high byte, then one of the low byte inside the bin that
//            holds the k-th largest key.  The pass that fills the first histogram also sums exp(x - max) over the finite logits and
//            counts the columns that rank before the target's (larger key, or equal key and lower index).
//   collect  every column above the k-th key is a candidate, the LOWEST-indexed columns equal to it fill the remaining places: a thread
//            owns a contiguous span of columns, one block-wide scan of packed (above, equal) counts gives every candidate its slot.
//   sort     the <= 64 candidates, as (key << 32 | ~column), sorted descending by one wave (bitonic, cross-lane exchanges): value
//            descending, then token ascending - ties are defined and the output is a function of the row alone.
// Non-finite logits are treated as absent throughout: lse is the log-sum-exp of the row's FINITE logits (-inf for a row without one), a
// row with fewer than k of them pads tok with -1 and logp with -inf, a target whose logit is not finite ranks V, a target outside
// [0, V) ranks -1.  Columns >= V of the padded row are loaded with their vector and masked.  No global atomics; every output word is
// written; deterministic.
#include <cmath>
#include <type_traits>

#include "gemm_launch.h"
#include "sample_common.h"

#define HT_MAX_K 64                       // = PLM_WAVE: one wave sorts the candidates
#define HT_ROW_LDS_BYTES (128 * 1024)     // LDS budget of a staged row: V <= 65536
#define HT_DEVICE_LDS_BYTES (160 * 1024)  // LDS of a gfx950 CU, the most one workgroup can have

struct HtScratch {
  unsigned h[256];          // the histogram of the current select level
  smp_u64 part[SMP_WAVES];  // sample_common.h's block reductions
  smp_u64 cand[HT_MAX_K];   // candidates: key << 32 | ~column; 0 = none
  float fsum[SMP_WAVES];
  unsigned res[2];
};
static_assert(HT_ROW_LDS_BYTES + sizeof(HtScratch) <= HT_DEVICE_LDS_BYTES, "a staged row, the histogram and the scratch share one CU's LDS");
static_assert(HT_MAX_K == PLM_WAVE && HT_MAX_K <= 256, "one wave sorts the candidates");

// the keys of the 8 columns col0 .. col0 + 7 of one 16-byte vector; a column >= V has key 0
template <class F>
__device__ __forceinline__ void ht_keys(const uint4 v, int col0, int V, F f) {
  auto pair = [&](unsigned w, int c) {  // two columns of one dword, the even one in the low half
    f(c < V ? smp_key(w & 0xFFFFu) : 0u, c);
    f(c + 1 < V ? smp_key(w >> 16) : 0u, c + 1);
  };
  pair(v.x, col0);
  pair(v.y, col0 + 2);
  pair(v.z, col0 + 4);
  pair(v.w, col0 + 6);
}

__device__ __forceinline__ void ht_clear(HtScratch& sc) {
  if (threadIdx.x < 256) sc.h[threadIdx.x] = 0u;
  __syncthreads();
}

// The bin of sc.h that holds the K-th largest counted key, when `above` keys are known to lie above every bin: (bin, keys above that bin).
// total = above + the histogram's sum (>= 1 required); K is cut to it.  Every thread gets the result, and sc.h may be cleared on return.
__device__ __forceinline__ uint2 ht_find(HtScratch& sc, unsigned K, unsigned above, unsigned& total) {
  const int tid = threadIdx.x;
  const unsigned c = tid < 256 ? sc.h[255 - tid] : 0u;  // thread order = descending bins
  smp_u64 tot;
  const unsigned incl = above + (unsigned)smp_block_scan(c, sc.part, tot);
  total = above + (unsigned)tot;
  const unsigned Kc = min(K, total);
  if (incl >= Kc && incl - c < Kc) {  // exactly one thread: incl does not decrease, and c > 0 here
    sc.res[0] = 255u - (unsigned)tid;
    sc.res[1] = incl - c;
  }
  __syncthreads();
  return make_uint2(sc.res[0], sc.res[1]);
}

// Radix select: the K-th largest (K cut to their number, total >= 1) of the 16-bit keys visit(first, emit) hands to emit - it is called
// twice, first = std::true_type then std::false_type, and must present the same keys both times.  n_above = keys larger than the
// result.  sc.h is clear at entry and on return.
template <class Visit>
__device__ __forceinline__ unsigned ht_kth(HtScratch& sc, unsigned K, Visit visit, unsigned& n_above, unsigned& total) {
  visit(std::true_type{}, [&](unsigned key) { atomicAdd(&sc.h[key >> 8], 1u); });
  __syncthreads();
  const uint2 hi = ht_find(sc, K, 0u, total);
  ht_clear(sc);
  visit(std::false_type{}, [&](unsigned key) {
    if ((key >> 8) == hi.x) atomicAdd(&sc.h[key & 255u], 1u);
  });
  __syncthreads();
  unsigned t2;
  const uint2 lo = ht_find(sc, K, hi.y, t2);
  ht_clear(sc);
  n_above = lo.y;
  return (hi.x << 8) | lo.x;
}

template <bool ROW_IN_LDS>
__global__ __launch_bounds__(SMP_THREADS) void head_topk_rows_kernel(const uint16_t* __restrict__ logits, int64_t ld,
                                                                     const int64_t* __restrict__ targets, HeadTopkOut out, int k, int V) {
  __shared__ uint4 s_row[ROW_IN_LDS ? HT_ROW_LDS_BYTES / 16 : 1];
  __shared__ HtScratch sc;

  const int tid = threadIdx.x;
  const int64_t r = blockIdx.x;
  const uint4* grow = reinterpret_cast<const uint4*>(logits + r * ld);
  const int nvec = (V + 7) >> 3;  // (ld = 8 * nvec at least: the last vector lies inside the row)
  auto vec = [&](int i) -> uint4 {
    if constexpr (ROW_IN_LDS) return s_row[i];
    else return grow[i];
  };

  // stage + the maxima
  unsigned tmax = 0u;
  for (int i = tid; i < nvec; i += SMP_THREADS) {
    const uint4 v = grow[i];
    if constexpr (ROW_IN_LDS) s_row[i] = v;
    ht_keys(v, i * 8, V, [&](unsigned key, int) { tmax = max(tmax, key); });
  }
  if (tid < 256) sc.h[tid] = 0u;
  const unsigned kmax = (unsigned)smp_block_max(tmax, sc.part);  // its barriers publish the row and the cleared histogram

  const int64_t tg = targets ? targets[r] : -1;
  const bool tg_ok = tg >= 0 && tg < V;
  if (kmax == 0u) {  // no finite logit in the row
    if (tid < k) {
      out.tok[r * k + tid] = -1;
      out.logp[r * k + tid] = -INFINITY;
    }
    if (tid == 0) {
      if (out.lse) out.lse[r] = -INFINITY;
      if (out.rank) out.rank[r] = tg_ok ? V : -1;
    }
    return;
  }
  const float xmax = smp_value(kmax);

  // the bound: the k-th largest thread maximum, when k threads have one
  unsigned bound = SMP_KEY_LO;
  {
    unsigned above, n_thr;
    const unsigned kth_max = ht_kth(sc, (unsigned)k, [&](auto, auto emit) {
      if (tmax != 0u) emit(tmax);
    }, above, n_thr);
    if (n_thr >= (unsigned)k) bound = kth_max;
  }

  // the target's key; ~0: nothing ranks before it (no target, or its logit is not finite)
  unsigned kt = ~0u;
  if (tg_ok) {
    unsigned bits;
    if constexpr (ROW_IN_LDS) bits = reinterpret_cast<const uint16_t*>(s_row)[tg];
    else bits = logits[r * ld + tg];
    kt = smp_key(bits);
  }
  const bool tg_finite = tg_ok && kt != 0u;
  if (!tg_finite) kt = ~0u;
  const int tgc = (int)tg;

  // select; the first walk over the row also sums exp(x - max) and counts the columns before the target
  float s = 0.f;
  unsigned before = 0u;
  unsigned n_above, n_cand;
  const unsigned kth = ht_kth(sc, (unsigned)k, [&](auto first, auto emit) {
    for (int i = tid; i < nvec; i += SMP_THREADS)
      ht_keys(vec(i), i * 8, V, [&](unsigned key, int c) {
        if (key == 0u) return;
        if constexpr (decltype(first)::value) {
          s += __expf(smp_value(key) - xmax);
          before += (key > kt || (key == kt && c < tgc)) ? 1u : 0u;
        }
        if (key >= bound) emit(key);
      });
  }, n_above, n_cand);
  const unsigned Kc = min((unsigned)k, n_cand);  // >= 1: the candidates the row has

  // collect: thread t owns the vectors [t * vpt, (t + 1) * vpt); above-threshold columns fill 0 .. n_above - 1, the lowest-indexed equal
  // ones n_above .. Kc - 1, both in column order
  const int vpt = (nvec + SMP_THREADS - 1) / SMP_THREADS;
  const int v0 = min(nvec, tid * vpt), v1 = min(nvec, v0 + vpt);
  smp_u64 cnt = 0;
  for (int i = v0; i < v1; ++i)
    ht_keys(vec(i), i * 8, V, [&](unsigned key, int) { cnt += key > kth ? (1ull << 32) : (key == kth ? 1ull : 0ull); });
  if (tid < HT_MAX_K) sc.cand[tid] = 0ull;  // published by the scan's barriers
  smp_u64 total;
  const smp_u64 excl = smp_block_scan(cnt, sc.part, total) - cnt;
  if (cnt != 0ull) {
    smp_u64 pos = excl + n_above;  // the next places, packed as the counts are (one variable: two would be selected by address)
    for (int i = v0; i < v1; ++i)
      ht_keys(vec(i), i * 8, V, [&](unsigned key, int c) {
        if (key < kth) return;
        const unsigned at = key > kth ? (unsigned)(pos >> 32) : (unsigned)pos;
        pos += key > kth ? (1ull << 32) : 1ull;
        if (at < Kc) sc.cand[at] = ((smp_u64)key << 32) | (smp_u64)(~(unsigned)c);  // (an equal column past the Kc-th place is none)
      });
  }

  // the row's sums: fixed order (lanes by xor, then waves ascending)
  s = wave_sum(s);
  if (tid % PLM_WAVE == 0) sc.fsum[tid / PLM_WAVE] = s;
  before = (unsigned)smp_block_sum(before, sc.part);  // its barriers publish fsum and the candidates
  if (tid >= PLM_WAVE) return;
  float z = 0.f;
#pragma unroll
  for (int w = 0; w < SMP_WAVES; ++w) z += sc.fsum[w];
  const float lse = xmax + __logf(z);

  // wave 0: bitonic sort, descending (composite keys of real candidates are distinct; 0 = none sinks to the end)
  smp_u64 v = sc.cand[tid];
#pragma unroll
  for (int kk = 2; kk <= HT_MAX_K; kk <<= 1)
#pragma unroll
    for (int j = kk >> 1; j > 0; j >>= 1) {
      const smp_u64 o = __shfl_xor(v, j, PLM_WAVE);
      const bool keep_max = ((tid & kk) == 0) == ((tid & j) == 0);
      v = keep_max ? (v > o ? v : o) : (v < o ? v : o);
    }
  if (tid < k) {
    const bool real = v != 0ull;
    out.tok[r * k + tid] = real ? (int64_t)(~(unsigned)v) : -1;
    out.logp[r * k + tid] = real ? smp_value((unsigned)(v >> 32)) - lse : -INFINITY;
  }
  if (tid == 0) {
    if (out.lse) out.lse[r] = lse;
    if (out.rank) out.rank[r] = tg_ok ? (tg_finite ? (int)before : V) : -1;
  }
}

void plm_launch_head_topk_rows(const uint16_t* logits, int64_t ld, const int64_t* targets, const HeadTopkOut& out, int64_t k, int64_t rows,
                               int64_t V, hipStream_t s) {
  if (plm_cdiv(V, 8) * 16 <= HT_ROW_LDS_BYTES)
    hipLaunchKernelGGL(head_topk_rows_kernel<true>, dim3((unsigned)rows), dim3(SMP_THREADS), 0, s, logits, ld, targets, out, (int)k, (int)V);
  else
    hipLaunchKernelGGL(head_topk_rows_kernel<false>, dim3((unsigned)rows), dim3(SMP_THREADS), 0, s, logits, ld, targets, out, (int)k, (int)V);
}
