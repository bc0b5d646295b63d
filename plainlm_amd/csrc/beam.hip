// Beam-search selection and bookkeeping for gfx950: per prompt the 2G best (score[g] + logp[g][v], g, v) of G rows of
// bf16 logits, sorted by score descending, then beam ascending, then token ascending (plm_beam_select_bf16: two launches); the walk over
// them that fills the next G live beams, the finished pool, the histories and the next ancestor table (plm_beam_advance: one launch); and
// the backtrack of the best hypotheses (plm_beam_finalize: one launch).  Nothing is read back by any of them.
//
// beam_row_kernel, one 1024-thread workgroup per row.  The row's 2G best columns are the 2G largest order-preserving 16-bit keys
// (sample_common.h: equal values have equal keys, NaN and the infinities have key 0 and are never candidates).  The 2G-th largest key
// comes from a radix select over the key space - a 256-bin count histogram of the high byte, then one of the low byte inside the bin that
// holds it.  Every column above that key is a candidate, and so are the LOWEST-INDEXED columns equal to it, as many as are missing: a
// thread owns a contiguous chunk of columns and one block-wide scan of (above, equal) counts, packed into one 64-bit integer, gives every
// candidate its place.  The same pass that fills the first histogram sums the fixed-point weights smp_fix(x - x_max) into the integer Z:
// logp = (x - x_max) - ln(Z / scale) is then a function of the row's multiset of logits - no sum depends on arrival order.
// beam_merge_kernel, one workgroup per prompt: scores the rows' G * 2G <= 2048 candidates in fp32 and sorts them in LDS (bitonic) on a
// 64-bit composite key - the order-preserving bits of the score, then 63 - beam, then 2^26 - 1 - token - so the descending sort IS the
// stated order and exact ties need no second rule.  A beam whose score is not finite has no candidate; missing candidates are
// (-inf, -1, -1) at the end of the list.
#include <cmath>

#include "plm_device.h"
#include "sample_common.h"

#include "../../include/plainlm_hip.h"

#define BEAM_MAX 32                       // beams per prompt
#define BEAM_MAX_CAND (2 * BEAM_MAX)      // candidates per row and per prompt
#define BEAM_SORT_MAX (BEAM_MAX * BEAM_MAX_CAND)
#define BEAM_TOK_BITS 26                  // the composite key holds a token in 26 bits
#define BEAM_ROW_META 4                   // words per row behind its candidates: x_max, ln(Z / scale), the number of candidates, 0

// words of workspace per row: 2G keys, 2G tokens, the meta words
static inline size_t beam_row_words(int64_t G) { return (size_t)(4 * G + BEAM_ROW_META); }

__global__ __launch_bounds__(SMP_THREADS) void beam_row_kernel(const uint16_t* __restrict__ logits, int64_t ld, unsigned* __restrict__ ws, int K2,
                                                               float scale, int V) {
  __shared__ unsigned s_h1[256];
  __shared__ unsigned s_h2[256];
  __shared__ smp_u64 s_part[SMP_WAVES];
  __shared__ unsigned s_res[3];

  const int tid = threadIdx.x;
  const uint16_t* row = logits + (int64_t)blockIdx.x * ld;
  unsigned* out = ws + (size_t)blockIdx.x * (2 * K2 + BEAM_ROW_META);

  unsigned kmax = 0;
  for (int i = tid; i < V; i += SMP_THREADS) kmax = max(kmax, smp_key(row[i]));
  if (tid < 256) {
    s_h1[tid] = 0u;
    s_h2[tid] = 0u;
  }
  kmax = (unsigned)smp_block_max(kmax, s_part);  // its barriers publish the cleared histograms
  for (int i = tid; i < 2 * K2; i += SMP_THREADS) out[i] = 0u;  // key 0: no candidate (every word of the row's workspace is written)
  if (kmax == 0u) {  // no finite logit in the row
    if (tid < BEAM_ROW_META) out[2 * K2 + tid] = 0u;
    return;
  }
  const float xmax = smp_value(kmax);

  // the high-byte histogram of every finite logit, and Z
  smp_u64 z = 0;
  for (int i = tid; i < V; i += SMP_THREADS) {
    const unsigned k = smp_key(row[i]);
    if (k == 0u) continue;
    atomicAdd(&s_h1[k >> 8], 1u);
    z += smp_fix(smp_value(k) - xmax, SMP_LOG2E, scale);
  }
  z = smp_block_sum(z, s_part);  // >= scale: the maximum weighs exp(0) = 1
  if (tid == 0) {
    unsigned total = 0;
    for (int b = 0; b < 256; ++b) total += s_h1[b];
    const unsigned K = min((unsigned)K2, total);  // >= 1
    unsigned acc = 0;
    int b = 255;
    for (; b > 0; --b) {
      if (acc + s_h1[b] >= K) break;
      acc += s_h1[b];
    }
    s_res[0] = (unsigned)b;  // the bin of the K-th largest key
    s_res[1] = acc;          // keys in the bins above it
    s_res[2] = K;
  }
  __syncthreads();
  const unsigned b1 = s_res[0], above1 = s_res[1], K = s_res[2];
  for (int i = tid; i < V; i += SMP_THREADS) {
    const unsigned k = smp_key(row[i]);
    if (k != 0u && (k >> 8) == b1) atomicAdd(&s_h2[k & 255u], 1u);
  }
  __syncthreads();
  if (tid == 0) {
    unsigned acc = above1;
    int b = 255;
    for (; b > 0; --b) {
      if (acc + s_h2[b] >= K) break;
      acc += s_h2[b];
    }
    s_res[0] = (b1 << 8) | (unsigned)b;  // the K-th largest key
    s_res[1] = acc;                      // keys above it: < K
  }
  __syncthreads();
  const unsigned kth = s_res[0], n_above = s_res[1];

  // places: thread t owns columns [t * chunk, (t + 1) * chunk); above-threshold columns fill 0 .. n_above - 1, the lowest-indexed equal
  // ones n_above .. K - 1, both in column order
  const int chunk = (V + SMP_THREADS - 1) / SMP_THREADS;
  const int c0 = min(V, tid * chunk), c1 = min(V, c0 + chunk);
  smp_u64 cnt = 0;
  for (int i = c0; i < c1; ++i) {
    const unsigned k = smp_key(row[i]);
    cnt += k > kth ? (1ull << 32) : (k == kth ? 1ull : 0ull);
  }
  smp_u64 total;
  const smp_u64 excl = smp_block_scan(cnt, s_part, total) - cnt;
  unsigned pa = (unsigned)(excl >> 32), pe = n_above + (unsigned)(excl & 0xFFFFFFFFull);
  for (int i = c0; i < c1; ++i) {
    const unsigned k = smp_key(row[i]);
    unsigned at = K;
    if (k > kth) at = pa++;
    else if (k == kth) at = pe++;
    if (at < K) {  // (an equal column past the K-th place is no candidate; K <= K2)
      out[at] = k;
      out[K2 + at] = (unsigned)i;
    }
  }
  if (tid == 0) {
    out[2 * K2] = __float_as_uint(xmax);
    out[2 * K2 + 1] = __float_as_uint(logf((float)((double)z / (double)scale)));
    out[2 * K2 + 2] = K;
    out[2 * K2 + 3] = 0u;
  }
}

// order-preserving bits of a finite fp32 (never 0)
__device__ __forceinline__ unsigned beam_ord(float v) {
  const unsigned u = __float_as_uint(v + 0.f);  // -0 -> +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float beam_unord(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }

__global__ __launch_bounds__(SMP_THREADS) void beam_merge_kernel(const unsigned* __restrict__ ws, const float* __restrict__ score,
                                                                 float* __restrict__ cand_score, int32_t* __restrict__ cand_beam,
                                                                 int32_t* __restrict__ cand_tok, int rpp, int K2, int n2) {
  __shared__ smp_u64 s_key[BEAM_SORT_MAX];
  const int tid = threadIdx.x;
  const int64_t p = blockIdx.x;
  const int n_in = rpp * K2;
  for (int i = tid; i < n2; i += SMP_THREADS) {
    smp_u64 ck = 0ull;
    if (i < n_in) {
      const int g = i / K2, e = i - g * K2;
      const unsigned* r = ws + (size_t)(p * rpp + g) * (2 * K2 + BEAM_ROW_META);
      const float sc0 = score[p * rpp + g];
      if (e < (int)r[2 * K2 + 2] && fabsf(sc0) < INFINITY) {  // (a NaN score fails the comparison too)
        const float logp = (smp_value(r[e]) - __uint_as_float(r[2 * K2])) - __uint_as_float(r[2 * K2 + 1]);
        const float sc = sc0 + logp;
        if (fabsf(sc) < INFINITY)
          ck = ((smp_u64)beam_ord(sc) << 32) | ((smp_u64)(63 - g) << BEAM_TOK_BITS) | (smp_u64)(((1u << BEAM_TOK_BITS) - 1u) - r[K2 + e]);
      }
    }
    s_key[i] = ck;
  }
  __syncthreads();
  // bitonic sort, descending (composite keys of real candidates are distinct; 0 = none sinks to the end)
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += SMP_THREADS) {
        const int x = i ^ j;
        if (x > i) {
          const smp_u64 a = s_key[i], b = s_key[x];
          const bool desc = (i & k) == 0;
          if (desc ? a < b : a > b) {
            s_key[i] = b;
            s_key[x] = a;
          }
        }
      }
      __syncthreads();
    }
  if (tid < K2) {
    const smp_u64 ck = s_key[tid];  // K2 <= n2
    const unsigned lo = (unsigned)ck;
    const bool real = ck != 0ull;
    cand_score[p * K2 + tid] = real ? beam_unord((unsigned)(ck >> 32)) : -INFINITY;
    cand_beam[p * K2 + tid] = real ? 63 - (int)(lo >> BEAM_TOK_BITS) : -1;
    cand_tok[p * K2 + tid] = real ? (int)(((1u << BEAM_TOK_BITS) - 1u) - (lo & ((1u << BEAM_TOK_BITS) - 1u))) : -1;
  }
}

extern "C" size_t plm_beam_select_workspace_bytes(int64_t rows, int64_t G) {
  if (rows < 1 || rows >= ((int64_t)1 << 26) || G < 1 || G > BEAM_MAX) return 0;
  return ((size_t)rows * beam_row_words(G) * 4 + 15) / 16 * 16;
}

extern "C" int plm_beam_select_bf16(const uint16_t* logits, int64_t ld, const float* score, float* cand_score, int32_t* cand_beam,
                                    int32_t* cand_tok, int64_t P, int64_t rows_per_prompt, int64_t G, int64_t V, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  const char* fn = "plm_beam_select_bf16";
  PLM_REQUIRE(logits && score && cand_score && cand_beam && cand_tok && workspace, "%s: null pointer", fn);
  PLM_REQUIRE(G >= 1 && G <= BEAM_MAX, "%s: G=%ld beams per prompt unsupported (1 .. %d)", fn, (long)G, BEAM_MAX);
  PLM_REQUIRE(rows_per_prompt >= 1 && rows_per_prompt <= G, "%s: rows_per_prompt=%ld must be in [1, G=%ld]", fn, (long)rows_per_prompt, (long)G);
  PLM_REQUIRE(P >= 1 && P * rows_per_prompt < ((int64_t)1 << 26), "%s: bad shape P=%ld", fn, (long)P);
  PLM_REQUIRE(V >= 2 * G && V <= ((int64_t)1 << BEAM_TOK_BITS) && ld >= V, "%s: bad shape V=%ld ld=%ld (need 2*G <= V <= 2^%d and ld >= V)", fn, (long)V,
              (long)ld, BEAM_TOK_BITS);
  PLM_REQUIRE((reinterpret_cast<uintptr_t>(logits) & 1) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
              "%s: logits must be 2-byte aligned, the workspace 16-byte aligned", fn);
  const int64_t rows = P * rows_per_prompt;
  const size_t need = plm_beam_select_workspace_bytes(rows, G);
  if (workspace_bytes < need) {
    plm_set_error("%s: workspace of %zu bytes required, %zu given", fn, need, workspace_bytes);
    return PLM_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const int K2 = (int)(2 * G);
  int n2 = 2;
  while (n2 < rows_per_prompt * K2) n2 <<= 1;  // <= BEAM_SORT_MAX
  unsigned* ws = static_cast<unsigned*>(workspace);
  hipLaunchKernelGGL(beam_row_kernel, dim3((unsigned)rows), dim3(SMP_THREADS), 0, s, logits, ld, ws, K2, smp_host_scale(V), (int)V);
  hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)P), dim3(SMP_THREADS), 0, s, ws, score, cand_score, cand_beam, cand_tok, (int)rows_per_prompt, K2,
                     n2);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

// ---- the walk over a prompt's sorted candidates ----------------------------------------------------------------------------------------
// The finished pool of a prompt: up to G hypotheses, pool_f [P, G, 2] = (normalised score, raw score), pool_i [P, G, 3] = (length, the step
// the backtrack starts at, the beam it starts at), pool_n [P].  An EOS hypothesis found at step t below parent b: length t + 1 (EOS
// counted), backtrack from (t - 1, b); a live beam n that enters at the end: length N, backtrack from (N - 1, n).
struct BeamPool {
  float* f;
  int32_t* i;
  int32_t* n;
};

__device__ __forceinline__ float beam_norm(float score, int len, float length_penalty) { return score / powf((float)len, length_penalty); }

// keep the G best by normalised score; an equal newcomer does not displace
__device__ void beam_pool_insert(float* pf, int32_t* pi, int32_t& pn, int G, float norm, float raw, int len, int step, int beam) {
  int at = pn;
  if (pn >= G) {
    at = 0;
    for (int e = 1; e < G; ++e)
      if (pf[2 * e] < pf[2 * at]) at = e;  // the worst; the first of equals
    if (!(norm > pf[2 * at])) return;
  } else {
    pn += 1;
  }
  pf[2 * at] = norm;
  pf[2 * at + 1] = raw;
  pi[3 * at] = len;
  pi[3 * at + 1] = step;
  pi[3 * at + 2] = beam;
}

__global__ __launch_bounds__(256) void beam_advance_kernel(const float* __restrict__ cand_score, const int32_t* __restrict__ cand_beam,
                                                           const int32_t* __restrict__ cand_tok, const uint8_t* __restrict__ anc_in,
                                                           uint8_t* __restrict__ anc_out, int64_t* __restrict__ tok_next, float* __restrict__ score_out,
                                                           int32_t* __restrict__ parent, int32_t* __restrict__ tok_hist, int32_t* __restrict__ par_hist,
                                                           BeamPool pool, int32_t* __restrict__ done, int G, int N, int t, int eos_id,
                                                           float length_penalty, int early_stopping) {
  __shared__ int s_par[BEAM_MAX];
  const int64_t p = blockIdx.x;
  if (threadIdx.x == 0) {
    float* pf = pool.f + p * G * 2;
    int32_t* pi = pool.i + p * G * 3;
    int32_t pn = pool.n[p];
    const bool frozen = done[p] != 0;
    int n = 0;
    for (int r = 0; r < 2 * G && n < G; ++r) {
      const int b = cand_beam[p * 2 * G + r], v = cand_tok[p * 2 * G + r];
      if (b < 0) break;  // no more candidates
      const float sc = cand_score[p * 2 * G + r];
      if (eos_id >= 0 && v == eos_id) {
        if (r < G && !frozen) beam_pool_insert(pf, pi, pn, G, beam_norm(sc, t + 1, length_penalty), sc, t + 1, t - 1, b);
        continue;
      }
      tok_next[p * G + n] = v;
      score_out[p * G + n] = sc;
      s_par[n] = b;
      ++n;
    }
    const float best_live = n > 0 ? score_out[p * G] : -INFINITY;
    for (; n < G; ++n) {  // a dead beam: no candidate was left for it; its score gives it no candidate later either
      tok_next[p * G + n] = eos_id >= 0 ? eos_id : 0;
      score_out[p * G + n] = -INFINITY;
      s_par[n] = 0;
    }
    for (int e = 0; e < G; ++e) {
      parent[p * G + e] = s_par[e];
      tok_hist[(p * N + t) * G + e] = (int32_t)tok_next[p * G + e];
      par_hist[(p * N + t) * G + e] = s_par[e];
    }
    if (!frozen) {
      pool.n[p] = pn;
      if (pn >= G) {
        float worst = pf[0];
        for (int e = 1; e < G; ++e) worst = fminf(worst, pf[2 * e]);
        if (early_stopping || !(beam_norm(best_live, t + 1, length_penalty) > worst)) done[p] = 1;
      }
    }
  }
  __syncthreads();
  // the next ancestor table: beam n continues its parent's history and owns row t of its own slot
  for (int i = threadIdx.x; i < G * (t + 1); i += blockDim.x) {
    const int n = i / (t + 1), j = i - n * (t + 1);
    anc_out[(p * G + n) * N + j] = j < t ? anc_in[(p * G + s_par[n]) * N + j] : (uint8_t)n;
  }
}

extern "C" int plm_beam_advance(const float* cand_score, const int32_t* cand_beam, const int32_t* cand_tok, const uint8_t* anc_in, uint8_t* anc_out,
                                int64_t* tok_next, float* score_out, int32_t* parent, int32_t* tok_hist, int32_t* par_hist, float* pool_f,
                                int32_t* pool_i, int32_t* pool_n, int32_t* done, int64_t P, int64_t G, int64_t N, int64_t t, int64_t eos_id,
                                float length_penalty, int early_stopping, void* stream) {
  const char* fn = "plm_beam_advance";
  PLM_REQUIRE(cand_score && cand_beam && cand_tok && anc_in && anc_out && tok_next && score_out && parent && tok_hist && par_hist && pool_f && pool_i &&
                  pool_n && done,
              "%s: null pointer", fn);
  PLM_REQUIRE(anc_in != anc_out, "%s: anc_in and anc_out must be the two halves of a ping-pong pair (parents repeat: no in-place gather)", fn);
  PLM_REQUIRE(G >= 1 && G <= BEAM_MAX, "%s: G=%ld beams per prompt unsupported (1 .. %d)", fn, (long)G, BEAM_MAX);
  PLM_REQUIRE(P >= 1 && P < ((int64_t)1 << 26) && N >= 1 && N < ((int64_t)1 << 24) && t >= 0 && t < N, "%s: bad shape P=%ld N=%ld t=%ld (0 <= t < N)", fn,
              (long)P, (long)N, (long)t);
  PLM_REQUIRE(eos_id >= -1 && eos_id < ((int64_t)1 << BEAM_TOK_BITS), "%s: eos_id %ld out of range (-1 = none)", fn, (long)eos_id);
  PLM_REQUIRE(std::isfinite(length_penalty), "%s: length_penalty must be finite", fn);
  hipLaunchKernelGGL(beam_advance_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, cand_score, cand_beam, cand_tok, anc_in, anc_out, tok_next,
                     score_out, parent, tok_hist, par_hist, BeamPool{pool_f, pool_i, pool_n}, done, (int)G, (int)N, (int)t, (int)eos_id, length_penalty,
                     early_stopping);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

// ---- the end: live beams of an unfinished prompt enter the pool, the best R hypotheses are backtracked ----------------------------------------
__global__ __launch_bounds__(64) void beam_finalize_kernel(const float* __restrict__ score, const int32_t* __restrict__ tok_hist,
                                                           const int32_t* __restrict__ par_hist, BeamPool pool, const int32_t* __restrict__ done,
                                                           int64_t* __restrict__ tokens, int32_t* __restrict__ lengths, float* __restrict__ scores, int G,
                                                           int N, int n_steps, int R, int eos_id, int pad_id, float length_penalty) {
  __shared__ float s_f[BEAM_MAX * 2];
  __shared__ int32_t s_i[BEAM_MAX * 3];
  __shared__ int s_pick[BEAM_MAX];
  const int64_t p = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid == 0) {  // a copy of the pool: the call changes no state
    int32_t pn = pool.n[p];
    for (int e = 0; e < pn; ++e) {
      s_f[2 * e] = pool.f[(p * G + e) * 2];
      s_f[2 * e + 1] = pool.f[(p * G + e) * 2 + 1];
      for (int c = 0; c < 3; ++c) s_i[3 * e + c] = pool.i[(p * G + e) * 3 + c];
    }
    if (done[p] == 0)
      for (int n = 0; n < G; ++n) {
        const float sc = score[p * G + n];
        if (fabsf(sc) < INFINITY) beam_pool_insert(s_f, s_i, pn, G, beam_norm(sc, n_steps, length_penalty), sc, n_steps, n_steps - 1, n);
      }
    unsigned taken = 0u;  // best first; among equals the earlier entry
    for (int r = 0; r < R; ++r) {
      int at = -1;
      for (int e = 0; e < pn; ++e)
        if (!((taken >> e) & 1u) && (at < 0 || s_f[2 * e] > s_f[2 * at])) at = e;
      s_pick[r] = at;
      if (at >= 0) taken |= 1u << at;
    }
  }
  __syncthreads();
  for (int r = tid; r < R; r += blockDim.x) {
    const int at = s_pick[r];
    int64_t* out = tokens + (p * R + r) * N;
    for (int j = 0; j < N; ++j) out[j] = pad_id;
    if (at < 0) {  // fewer hypotheses than asked for
      lengths[p * R + r] = 0;
      scores[p * R + r] = -INFINITY;
      continue;
    }
    const int len = s_i[3 * at];
    int step = s_i[3 * at + 1], b = s_i[3 * at + 2];
    if (step == len - 2) out[len - 1] = eos_id;  // an EOS hypothesis: its last token
    for (; step >= 0; --step) {
      out[step] = tok_hist[(p * N + step) * G + b];
      b = par_hist[(p * N + step) * G + b];
      b = b < 0 ? 0 : (b >= G ? G - 1 : b);
    }
    lengths[p * R + r] = len;
    scores[p * R + r] = s_f[2 * at];
  }
}

extern "C" int plm_beam_finalize(const float* score, const int32_t* tok_hist, const int32_t* par_hist, const float* pool_f, const int32_t* pool_i,
                                 const int32_t* pool_n, const int32_t* done, int64_t* tokens, int32_t* lengths, float* scores, int64_t P, int64_t G,
                                 int64_t N, int64_t n_steps, int64_t R, int64_t eos_id, int64_t pad_id, float length_penalty, void* stream) {
  const char* fn = "plm_beam_finalize";
  PLM_REQUIRE(score && tok_hist && par_hist && pool_f && pool_i && pool_n && done && tokens && lengths && scores, "%s: null pointer", fn);
  PLM_REQUIRE(G >= 1 && G <= BEAM_MAX && R >= 1 && R <= G, "%s: G=%ld, num_return=%ld unsupported (1 <= num_return <= G <= %d)", fn, (long)G, (long)R,
              BEAM_MAX);
  PLM_REQUIRE(P >= 1 && P < ((int64_t)1 << 26) && N >= 1 && N < ((int64_t)1 << 24) && n_steps >= 1 && n_steps <= N,
              "%s: bad shape P=%ld N=%ld n_steps=%ld (1 <= n_steps <= N)", fn, (long)P, (long)N, (long)n_steps);
  PLM_REQUIRE(eos_id >= -1 && eos_id < ((int64_t)1 << BEAM_TOK_BITS), "%s: eos_id %ld out of range (-1 = none)", fn, (long)eos_id);
  PLM_REQUIRE(std::isfinite(length_penalty), "%s: length_penalty must be finite", fn);
  hipLaunchKernelGGL(beam_finalize_kernel, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, score, tok_hist, par_hist,
                     BeamPool{const_cast<float*>(pool_f), const_cast<int32_t*>(pool_i), const_cast<int32_t*>(pool_n)}, done, tokens, lengths, scores,
                     (int)G, (int)N, (int)n_steps, (int)R, (int)eos_id, (int)pad_id, length_penalty);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}
