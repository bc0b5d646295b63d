// Prompt-lookup (n-gram) drafting on the device for gfx950: a sequence proposes its own continuation.  The tokens
// that followed the most recent earlier occurrence of its last few tokens are the draft - no draft model, no second cache.  Integers
// only; one workgroup per sequence, one launch per round: it appends what the previous round committed to the sequence's token history,
// searches the history, and copies the proposal out.  Nothing is read back and there is no workspace.
//
// The search is a block-wide maximum over one 64-bit key per candidate end e: (match length << 32) | e, so the longest match wins and,
// among equal lengths, the most recent one.  A match is compared backwards from the end, and the first comparison fails for most ends:
// the usual cost is one coalesced 8-byte load per history token, from lines the append of earlier rounds left in L2.
#include "plm_device.h"

#include "../../include/plainlm_hip.h"

#define LKP_THREADS 256
#define LKP_WAVES (LKP_THREADS / PLM_WAVE)
#define LKP_MAX_DRAFT 31  // generate.MAX_DRAFT: a chunk of k + 1 <= 32 rows is one wave's queries in attn_extend_kernel
#define LKP_MAX_NGRAM 16

typedef unsigned long long lkp_u64;

__global__ __launch_bounds__(LKP_THREADS) void lookup_draft_kernel(int64_t* __restrict__ hist, int64_t ld, int32_t* __restrict__ lens,
                                                                   const int64_t* __restrict__ add_tok, int64_t ld_add,
                                                                   const int32_t* __restrict__ n_add, int64_t* __restrict__ draft_tok,
                                                                   int32_t* __restrict__ n_prop, int32_t* __restrict__ match_len,
                                                                   int32_t* __restrict__ status, int k, int g_min, int g_max) {
  __shared__ int64_t s_suf[LKP_MAX_NGRAM];  // s_suf[t - 1] = hist[L - t]
  __shared__ lkp_u64 s_best[LKP_WAVES];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  int64_t* row = hist + b * ld;
  int64_t* prop = draft_tok + b * k;
  const int64_t L0 = lens[b];
  int64_t c = 0;
  if (add_tok != nullptr) {
    c = n_add != nullptr ? (int64_t)n_add[b] : ld_add;
    c = c < 0 ? 0 : (c > ld_add ? ld_add : c);
  }
  if (L0 < 0 || L0 + c > ld) {  // the whole block: the sequence is refused, nothing of it is stored and no history row is read
    if (tid < k) prop[tid] = 0;
    if (tid == 0) {
      n_prop[b] = 0;
      if (match_len != nullptr) match_len[b] = 0;
      *status = 1;
    }
    return;
  }
  // ---- append ---------------------------------------------------------------------------------------------------------------------
  for (int64_t i = tid; i < c; i += LKP_THREADS) row[L0 + i] = add_tok[b * ld_add + i];
  const int64_t L = L0 + c;
  const int gcap = (int)min((int64_t)g_max, L - 1);  // an end e <= L - 1 compares at most min(g_max, e) tokens
  __threadfence_block();
  __syncthreads();  // the appended tokens are visible to every thread of the block; every thread has read lens[b]
  if (tid == 0) lens[b] = (int32_t)L;
  if (tid < gcap) s_suf[tid] = row[L - 1 - tid];
  __syncthreads();
  // ---- search: ends e in [1, L - 1], m(e) = the number of t = 1, 2, .. with hist[e - t] == hist[L - t], up to min(g_max, e) ---------
  lkp_u64 best = 0;
  for (int64_t e = 1 + tid; e < L; e += LKP_THREADS) {
    const int cap = (int)min((int64_t)gcap, e);
    int m = 0;
    while (m < cap && row[e - 1 - m] == s_suf[m]) ++m;
    if (m >= g_min) {
      const lkp_u64 key = ((lkp_u64)m << 32) | (lkp_u64)e;
      best = key > best ? key : best;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const lkp_u64 t = __shfl_xor(best, o, PLM_WAVE);
    best = t > best ? t : best;
  }
  if (tid % PLM_WAVE == 0) s_best[tid / PLM_WAVE] = best;
  __syncthreads();
  best = 0;
#pragma unroll
  for (int w = 0; w < LKP_WAVES; ++w) best = s_best[w] > best ? s_best[w] : best;
  // ---- propose: an overlapped copy of period L - e, so that a loop shorter than k still yields k tokens ---------------------------------
  const int64_t e = (int64_t)(best & 0xFFFFFFFFull);
  const int64_t period = L - e;  // >= 1 for a winner (e <= L - 1)
  if (tid < k) prop[tid] = best != 0ull ? row[e + tid % period] : 0;
  if (tid == 0) {
    n_prop[b] = best != 0ull ? k : 0;
    if (match_len != nullptr) match_len[b] = (int32_t)(best >> 32);
  }
}

extern "C" int plm_lookup_draft_i64(int64_t* hist, int64_t ld, int32_t* lens, const int64_t* add_tok, int64_t ld_add, const int32_t* n_add,
                                    int64_t* draft_tok, int32_t* n_prop, int32_t* match_len, int32_t* status, int64_t B, int64_t k,
                                    int64_t g_min, int64_t g_max, void* stream) {
  PLM_REQUIRE(hist && lens && draft_tok && n_prop && status, "plm_lookup_draft_i64: null pointer");
  PLM_REQUIRE(add_tok || !n_add, "plm_lookup_draft_i64: n_add without add_tok");
  PLM_REQUIRE(k >= 1 && k <= LKP_MAX_DRAFT, "plm_lookup_draft_i64: k=%ld drafted tokens (need 1 <= k <= %d)", (long)k, LKP_MAX_DRAFT);
  PLM_REQUIRE(g_min >= 1 && g_min <= g_max && g_max <= LKP_MAX_NGRAM, "plm_lookup_draft_i64: ngram (%ld, %ld) (need 1 <= g_min <= g_max <= %d)",
              (long)g_min, (long)g_max, LKP_MAX_NGRAM);
  PLM_REQUIRE(B >= 1 && B < ((int64_t)1 << 31) && ld >= 1 && ld < ((int64_t)1 << 31) && (!add_tok || (ld_add >= 1 && ld_add < ((int64_t)1 << 31))),
              "plm_lookup_draft_i64: bad shape B=%ld ld=%ld ld_add=%ld (need 1 <= B < 2^31, 1 <= ld < 2^31 and, with add_tok, 1 <= ld_add < 2^31)",
              (long)B, (long)ld, (long)ld_add);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(hist) | reinterpret_cast<uintptr_t>(add_tok) | reinterpret_cast<uintptr_t>(draft_tok)) & 7) == 0,
              "plm_lookup_draft_i64: hist, add_tok and draft_tok must be 8-byte aligned");
  hipLaunchKernelGGL(lookup_draft_kernel, dim3((unsigned)B), dim3(LKP_THREADS), 0, (hipStream_t)stream, hist, ld, lens, add_tok, ld_add, n_add,
                     draft_tok, n_prop, match_len, status, (int)k, (int)g_min, (int)g_max);
  PLM_CHECK_LAUNCH("plm_lookup_draft_i64");
  return PLM_OK;
}
