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

// The search both kernels share, by the whole block: over the ends e in [1, e_end), m(e) = the number of t = 1, 2, .. with
// hist[e - t] == hist[L - t] (s_suf[t - 1]), up to min(gcap, e); returns the largest key (m << 32) | e with m >= g_min, 0 for none.
// Ends with a barrier, so s_best may be used again.
__device__ __forceinline__ lkp_u64 lkp_search(const int64_t* row, const int64_t* s_suf, lkp_u64* s_best, int64_t e_end, int gcap,
                                              int g_min, int tid) {
  lkp_u64 best = 0;
  for (int64_t e = 1 + tid; e < e_end; e += LKP_THREADS) {
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
  __syncthreads();
  return best;
}

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
  const lkp_u64 best = lkp_search(row, s_suf, s_best, L, gcap, g_min, tid);
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

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_lookup_draft_tree_i64: the same history handling and match rule, but the up to n_branch most recent ends of
// the longest match are kept and their continuations (k tokens each, the overlapped copy above) are merged into a trie of at most n rows:
// row 0 is the root (the sequence's newest token), equal tokens under one parent share a row, rows are in creation order (parent < row),
// the most recent match is inserted first.  The further ends come from the same search: the first winner's length is the maximum, so
// "the most recent end below the previous one with at least that length" is the next end of an equally long match.
// ---------------------------------------------------------------------------------------------------------------------------------
#define LKP_MAX_ROWS 32
#define LKP_MAX_BRANCH 8

__global__ __launch_bounds__(LKP_THREADS) void lookup_draft_tree_kernel(int64_t* __restrict__ hist, int64_t ld, int32_t* __restrict__ lens,
                                                                        const int64_t* __restrict__ add_tok, int64_t ld_add,
                                                                        const int32_t* __restrict__ n_add, int64_t* __restrict__ tok,
                                                                        int32_t* __restrict__ parent, int32_t* __restrict__ n_new,
                                                                        int32_t* __restrict__ match_len, int32_t* __restrict__ status, int n, int k,
                                                                        int n_branch, int g_min, int g_max) {
  __shared__ int64_t s_suf[LKP_MAX_NGRAM];
  __shared__ lkp_u64 s_best[LKP_WAVES];
  __shared__ int64_t s_tok[LKP_MAX_ROWS];
  __shared__ int s_par[LKP_MAX_ROWS];
  __shared__ int s_rows;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  int64_t* row = hist + b * ld;
  const int64_t L0 = lens[b];
  int64_t c = 0;
  if (add_tok != nullptr) {
    c = n_add != nullptr ? (int64_t)n_add[b] : ld_add;
    c = c < 0 ? 0 : (c > ld_add ? ld_add : c);
  }
  const bool refused = L0 < 0 || L0 + c > ld || L0 + c < 1;  // (block-uniform) no history row is read or written; an empty history has no root
  if (tid < LKP_MAX_ROWS) {
    s_tok[tid] = 0;
    s_par[tid] = -1;
  }
  if (tid == 0) s_rows = refused ? 0 : 1;
  lkp_u64 best = 0;
  if (!refused) {
    for (int64_t i = tid; i < c; i += LKP_THREADS) row[L0 + i] = add_tok[b * ld_add + i];
    const int64_t L = L0 + c;
    const int gcap = (int)min((int64_t)g_max, L - 1);
    __threadfence_block();
    __syncthreads();
    if (tid == 0) lens[b] = (int32_t)L;
    if (tid < gcap) s_suf[tid] = row[L - 1 - tid];
    __syncthreads();
    best = lkp_search(row, s_suf, s_best, L, gcap, g_min, tid);
    const int mlen = (int)(best >> 32);
    if (tid == 0) s_tok[0] = row[L - 1];
    lkp_u64 cur = best;
    for (int br = 0; br < n_branch && cur != 0ull; ++br) {  // (cur block-uniform)
      const int64_t e = (int64_t)(cur & 0xFFFFFFFFull);
      if (tid == 0) {  // the merge: one thread, at most n rows
        const int64_t period = L - e;
        int at = 0, rows = s_rows;
        for (int t = 0; t < k; ++t) {
          const int64_t x = row[e + t % period];
          int child = -1;
          for (int j = at + 1; j < rows; ++j)
            if (s_par[j] == at && s_tok[j] == x) {
              child = j;
              break;
            }
          if (child < 0) {
            if (rows >= n) break;
            child = rows++;
            s_tok[child] = x;
            s_par[child] = at;
          }
          at = child;
        }
        s_rows = rows;
      }
      cur = br + 1 < n_branch ? lkp_search(row, s_suf, s_best, e, gcap, mlen, tid) : 0ull;
    }
  } else if (tid == 0) {
    *status = 1;
  }
  __syncthreads();
  if (tid < n) {
    tok[b * n + tid] = s_tok[tid];
    parent[b * n + tid] = s_par[tid];
  }
  if (tid == 0) {
    n_new[b] = s_rows;
    if (match_len != nullptr) match_len[b] = (int32_t)(best >> 32);
  }
}

extern "C" int plm_lookup_draft_tree_i64(int64_t* hist, int64_t ld, int32_t* lens, const int64_t* add_tok, int64_t ld_add, const int32_t* n_add,
                                         int64_t* tok, int32_t* parent, int32_t* n_new, int32_t* match_len, int32_t* status, int64_t B, int64_t n,
                                         int64_t k, int64_t n_branch, int64_t g_min, int64_t g_max, void* stream) {
  const char* fn = "plm_lookup_draft_tree_i64";
  PLM_REQUIRE(hist && lens && tok && parent && n_new && status, "%s: null pointer", fn);
  PLM_REQUIRE(add_tok || !n_add, "%s: n_add without add_tok", fn);
  PLM_REQUIRE(n >= 1 && n <= LKP_MAX_ROWS && k >= 1 && k <= LKP_MAX_DRAFT && n_branch >= 1 && n_branch <= LKP_MAX_BRANCH,
              "%s: n=%ld rows, k=%ld tokens per branch, n_branch=%ld (need 1 <= n <= %d, 1 <= k <= %d, 1 <= n_branch <= %d)", fn, (long)n, (long)k,
              (long)n_branch, LKP_MAX_ROWS, LKP_MAX_DRAFT, LKP_MAX_BRANCH);
  PLM_REQUIRE(g_min >= 1 && g_min <= g_max && g_max <= LKP_MAX_NGRAM, "%s: ngram (%ld, %ld) (need 1 <= g_min <= g_max <= %d)", fn, (long)g_min,
              (long)g_max, LKP_MAX_NGRAM);
  PLM_REQUIRE(B >= 1 && B < ((int64_t)1 << 31) && ld >= 1 && ld < ((int64_t)1 << 31) && (!add_tok || (ld_add >= 1 && ld_add < ((int64_t)1 << 31))),
              "%s: bad shape B=%ld ld=%ld ld_add=%ld (need 1 <= B < 2^31, 1 <= ld < 2^31 and, with add_tok, 1 <= ld_add < 2^31)", fn, (long)B, (long)ld,
              (long)ld_add);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(hist) | reinterpret_cast<uintptr_t>(add_tok) | reinterpret_cast<uintptr_t>(tok)) & 7) == 0,
              "%s: hist, add_tok and tok must be 8-byte aligned", fn);
  hipLaunchKernelGGL(lookup_draft_tree_kernel, dim3((unsigned)B), dim3(LKP_THREADS), 0, (hipStream_t)stream, hist, ld, lens, add_tok, ld_add, n_add,
                     tok, parent, n_new, match_len, status, (int)n, (int)k, (int)n_branch, (int)g_min, (int)g_max);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}
