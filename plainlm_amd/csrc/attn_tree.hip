// Tree verification for lookup decoding on gfx950: one extend checks a TRIE of drafted continuations.  A chunk is
// n <= 32 rows per sequence; row 0 is the root (the newest committed token), parent[b, r] < r names row r's parent, and row r is a node at
// depth[r] = depth[parent[r]] + 1.  It is STORED at cache row lens0[b] + r and ROTATED at position lens0[b] + depth[r]; it attends the
// prefix keys [0, lens0[b]) and, of the chunk's keys, its ancestors and itself: anc[b, r], one bit per chunk row.
//
//   plm_tree_plan           parent -> depth, anc (one workgroup per sequence, thread r walks its own chain)
//   plm_attn_extend_tree    three launches over the partial layout of DESIGN.md section 21 with S_s = 1:
//                             prefix  attn_shared_prefix_kernel (attn_shared.hip) as it is: P = B, G = n, lens_p = lens0 - every node sees
//                                     every prefix key, the query row b*n + r is its p*G + g, and all four waves compute
//                             chunk   attn_tree_chunk_kernel below: the <= 32 chunk keys under the ancestor mask, one partial per row
//                             combine attn_cache_combine_kernel over S_p + 1 partials in key order
//   plm_tree_accept_greedy  the longest root-to-leaf path the target's greedy predictions follow (integers, one wave per sequence)
//   plm_kv_tree_commit      cache row lens0 + path[d] -> lens0 + d for the accepted depths, every layer in one launch
//
// attn_tree_chunk_kernel.  One wave per (sequence, head): the chunk is at most 32 keys by 32 queries, ONE 32x32 tile of
// v_mfma_f32_32x32x16_bf16, so there is no loop, no running maximum and no barrier.  S^T = K Q^T: K rows go from global memory straight
// into the A operand (lane (i, hi) loads 16 bytes of key row i at head dims ks*16 + hi*8, the prefix kernel's scheme), the lane's query
// is the B operand, so lane (r, hi) holds the scores of query r against keys mfma32_row(e, hi) and masks them with one shift of its own
// anc word.  fp32 statistics, the m_safe guard, bf16 P; V needs the transposed read (GenTile::cols) and goes through a 32-row LDS tile
// that only this wave touches (a wavefront-scope fence orders it); O^T += V^T P^T.  Row indices are clamped to the last valid chunk row,
// so a row at or beyond lens0 + c_b (stale, maybe NaN) never reaches LDS or an MFMA operand; rows r >= c_b write nothing.  No atomics:
// every partial has one writer.
// Built without packed fp32 VALU ops, as attn_shared.hip is (Makefile).
#include "attn_gen_tile.h"
#include "attn_cache.h"

#include "../../include/plainlm_hip.h"

#define TREE_MAX_ROWS 32
#define TREE_MAX_LAYERS 64  // cache pointers per plm_kv_tree_commit launch

__device__ __forceinline__ int tree_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_tree_plan: one wave per sequence, thread r < n owns row r
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void tree_plan_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ n_new,
                                                       int32_t* __restrict__ depth, uint32_t* __restrict__ anc, int32_t* __restrict__ status,
                                                       int n) {
  __shared__ int s_par[TREE_MAX_ROWS];
  const int b = blockIdx.x, r = threadIdx.x;
  const int cb = tree_clamp(n_new != nullptr ? n_new[b] : n, 0, n);
  const int p = r < n ? parent[(int64_t)b * n + r] : -1;
  // a real row's parent must be an earlier row (or -1: a root; row 0 must be one).  Rows at and beyond c_b are padding: never followed
  const bool bad = r < cb && (p < -1 || p >= r);
  if (r < TREE_MAX_ROWS) s_par[r] = p;
  __syncthreads();
  const bool refused = __ballot(bad) != 0ull;  // wave-uniform
  if (refused && r == 0) status[0] = 1;
  if (r >= n) return;
  int d = 0;
  uint32_t a = 0u;
  if (refused) {
    d = -1;  // what the append stages read at row 0: nothing of this sequence is stored
  } else if (r < cb) {
    a = 1u << r;
    int q = p;
    for (int step = 0; step < n && q >= 0; ++step) {  // q < its child < n: at most n - 1 steps, every s_par[q] was checked above
      a |= 1u << q;
      ++d;
      q = s_par[q];
    }
  }
  depth[(int64_t)b * n + r] = d;
  anc[(int64_t)b * n + r] = a;
}

extern "C" int plm_tree_plan(const int32_t* parent, const int32_t* n_new, int32_t* depth, uint32_t* anc, int32_t* status, int64_t B, int64_t n,
                             void* stream) {
  PLM_REQUIRE(parent && depth && anc && status, "plm_tree_plan: null pointer");
  PLM_REQUIRE(B >= 1 && B < ((int64_t)1 << 31) && n >= 1 && n <= TREE_MAX_ROWS, "plm_tree_plan: bad shape B=%ld n=%ld (need B >= 1, 1 <= n <= %d)",
              (long)B, (long)n, TREE_MAX_ROWS);
  hipLaunchKernelGGL(tree_plan_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, parent, n_new, depth, anc, status, (int)n);
  PLM_CHECK_LAUNCH("plm_tree_plan");
  return PLM_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_attn_extend_tree
// ---------------------------------------------------------------------------------------------------------------------------------
// wave-local ordering of LDS traffic (attn_shared.hip's shp_wave_sync: one wave's LDS instructions execute in order)
__device__ __forceinline__ void tree_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workspace: ml fp32 [B*n*nh, Stot, 2] then acc fp32 [B*n*nh, Stot, hd]; this kernel fills split `part_off` (= S_p, the suffix slot) of
// every (row b*n + r, head) with r < c_b.
template <int HD>
__global__ __launch_bounds__(64) void attn_tree_chunk_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ kv, int64_t ld_kv,
                                                             const int32_t* __restrict__ lens0, const int32_t* __restrict__ n_new,
                                                             const uint32_t* __restrict__ anc, float* __restrict__ ws_ml,
                                                             float* __restrict__ ws_acc, int n, int Tmax, int nh, int Stot, int part_off,
                                                             float scale) {
  using TL = GenTile<HD>;
  constexpr int NKS = HD / 16, NDB = HD / 32, CPR = HD / 8;
  __shared__ __attribute__((aligned(16))) char sV[32 * TL::ROWB];  // the chunk's V rows; this wave is the only one here
  const int h = (int)(blockIdx.x % nh), b = (int)(blockIdx.x / nh);
  const int dm = nh * HD;
  const int lane = threadIdx.x, l31 = lane & 31, hi = lane >> 5;

  const int l0 = tree_clamp(lens0[b], 0, Tmax);
  const int cb = tree_clamp(n_new != nullptr ? n_new[b] : n, 0, n);
  const int ck = l0 + cb <= Tmax ? cb : 0;  // chunk keys l0 .. l0 + ck - 1; a chunk that did not fit was not stored: it has no keys
  if (cb == 0) return;                // no row of this sequence writes anything (wave-uniform)
  const int r = l31;
  const bool valid = r < cb;
  // the keys this lane's query may see: its ancestors and itself, among the keys that exist
  const uint32_t seen = valid && ck > 0 ? anc[(int64_t)b * n + r] & (ck >= 32 ? 0xFFFFFFFFu : ((1u << ck) - 1u)) : 0u;

  const float c2 = scale * GLOG2E;
  f32x16_t o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) gzero16(o[db]);
  float m = -INFINITY, ltot = 0.f;
  if (ck > 0) {  // wave-uniform
    const uint16_t* kbase = kv + ((int64_t)b * Tmax + l0) * ld_kv + h * HD;  // + j * ld_kv: k of chunk key j; + dm: its v
    bf16x8_t qf[NKS], kf[NKS];
    {
      const uint16_t* kr = kbase + (int64_t)min(l31, ck - 1) * ld_kv + hi * 8;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        kf[ks] = ld_bf16x8(kr + ks * 16);
        qf[ks] = valid ? ld_bf16x8(q + ((int64_t)b * n + r) * dm + h * HD + ks * 16 + hi * 8) : zero_bf16x8();
      }
    }
#pragma unroll
    for (int it = 0; it < CPR / 2; ++it) {  // 32 rows of CPR 16-byte chunks over 64 lanes
      const int c = it * 64 + lane, vr = c / CPR, k = c - vr * CPR;
      *reinterpret_cast<bf16x8_t*>(sV + vr * TL::ROWB + k * 16) = ld_bf16x8(kbase + dm + (int64_t)min(vr, ck - 1) * ld_kv + k * 8);
    }
    tree_wave_sync();
    f32x16_t s;
    gzero16(s);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) s = mfma32(kf[ks], qf[ks], s);
    float tmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (((seen >> mfma32_row(e, hi)) & 1u) == 0u) s[e] = -INFINITY;
      tmax = fmaxf(tmax, s[e]);
    }
    {
      float t_lo, t_hi;
      half_pair(tmax, t_lo, t_hi);
      tmax = fmaxf(t_lo, t_hi);
    }
    m = tmax * c2;  // -inf for a query that sees no chunk key
    const float m_safe = (m == -INFINITY) ? 0.f : m;
    float psum = 0.f;
    bf16x8_t pf[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float pe = __builtin_amdgcn_exp2f(__builtin_fmaf(s[e], c2, -m_safe));
      psum += pe;
      pf[e >> 3][e & 7] = f2bf(pe);
    }
    float l_lo, l_hi;
    half_pair(psum, l_lo, l_hi);
    ltot = l_lo + l_hi;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int u = 0; u < 2; ++u) o[db] = mfma32(TL::cols(sV, db, u * 16 + 4 * hi, lane), pf[u], o[db]);
  }
  if (!valid) return;  // a row at or beyond c_b: no partial
  const int64_t part = (((int64_t)b * n + r) * nh + h) * Stot + part_off;  // no key seen: (m = -inf, l = 0, acc = 0), an empty partial
  if (hi == 0) {
    ws_ml[part * 2] = m;
    ws_ml[part * 2 + 1] = ltot;
  }
  float* arow = ws_acc + part * HD;  // (8-byte aligned: acc starts 8 * parts bytes into the workspace)
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float* dst = arow + db * 32 + 8 * g + 4 * hi;
      *reinterpret_cast<float2*>(dst) = make_float2(o[db][4 * g], o[db][4 * g + 1]);
      *reinterpret_cast<float2*>(dst + 2) = make_float2(o[db][4 * g + 2], o[db][4 * g + 3]);
    }
}

static bool tree_shape_ok(int64_t B, int64_t n, int64_t nh, int64_t hd, int64_t Tmax, int splits) {
  return n >= 1 && n <= TREE_MAX_ROWS && cache_shape_ok(B, 1, nh, hd, Tmax) && cache_shape_ok(B * n, 1, nh, hd, Tmax) && splits >= 0 &&
         splits <= CACHE_MAX_SPLITS;
}

// the prefix splits follow plm_attn_decode_shared's rule at P = B, G = n; the chunk adds one partial: shapes and splits alone
extern "C" size_t plm_attn_extend_tree_workspace_bytes(int64_t B, int64_t n, int64_t nh, int64_t hd, int64_t Tmax, int splits) {
  if (!tree_shape_ok(B, n, nh, hd, Tmax, splits)) return 0;
  return cache_ws_bytes(B * n, 1, nh, hd, shared_resolve_splits_p(B, n, nh, Tmax, splits) + 1);
}

template <int HD>
static void tree_chunk_launch(const uint16_t* q, const uint16_t* kv, int64_t ld_kv, const int32_t* lens0, const int32_t* n_new, const uint32_t* anc,
                              float* ws_ml, float* ws_acc, int64_t B, int64_t n, int64_t Tmax, int64_t nh, int Stot, hipStream_t s) {
  hipLaunchKernelGGL(attn_tree_chunk_kernel<HD>, dim3((unsigned)(B * nh)), dim3(64), 0, s, q, kv, ld_kv, lens0, n_new, anc, ws_ml, ws_acc, (int)n,
                     (int)Tmax, (int)nh, Stot, Stot - 1, 1.f / sqrtf((float)HD));
}

extern "C" int plm_attn_extend_tree(const uint16_t* q, const uint16_t* kv, int64_t ld_kv, const int32_t* lens0, const int32_t* n_new,
                                    const uint32_t* anc, uint16_t* out, float* lse, int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd,
                                    int splits, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "plm_attn_extend_tree";
  PLM_REQUIRE(q && kv && lens0 && anc && out && workspace, "%s: null pointer", fn);
  PLM_REQUIRE(hd == 32 || hd == 64 || hd == 128, "%s: head_dim %ld unsupported (32, 64, 128)", fn, (long)hd);
  PLM_REQUIRE(splits >= 0 && splits <= CACHE_MAX_SPLITS, "%s: splits=%d out of range (0 = automatic, 1..%d forced)", fn, splits, CACHE_MAX_SPLITS);
  PLM_REQUIRE(tree_shape_ok(B, n, nh, hd, Tmax, splits), "%s: bad shape B=%ld n=%ld Tmax=%ld nh=%ld (1 <= n <= %d)", fn, (long)B, (long)n, (long)Tmax,
              (long)nh, TREE_MAX_ROWS);
  PLM_REQUIRE(ld_kv >= 2 * nh * hd && ld_kv % 8 == 0, "%s: the cache's row stride must be a multiple of 8 and at least 2*nh*hd", fn);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(kv) | reinterpret_cast<uintptr_t>(out) |
                reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
              "%s: q, kv, out and the workspace must be 16-byte aligned", fn);
  const int Sp = shared_resolve_splits_p(B, n, nh, Tmax, splits), Stot = Sp + 1;
  const size_t need = cache_ws_bytes(B * n, 1, nh, hd, Stot);
  if (workspace_bytes < need) {
    plm_set_error("%s: workspace of %zu bytes required, %zu given", fn, need, workspace_bytes);
    return PLM_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* ws_ml = static_cast<float*>(workspace);
  float* ws_acc = ws_ml + (size_t)B * n * nh * Stot * 2;
  shared_prefix_launch(q, kv, ld_kv, lens0, ws_ml, ws_acc, B, n, Tmax, nh, hd, Sp, Stot, s);
  if (hd == 32) tree_chunk_launch<32>(q, kv, ld_kv, lens0, n_new, anc, ws_ml, ws_acc, B, n, Tmax, nh, Stot, s);
  else if (hd == 64) tree_chunk_launch<64>(q, kv, ld_kv, lens0, n_new, anc, ws_ml, ws_acc, B, n, Tmax, nh, Stot, s);
  else tree_chunk_launch<128>(q, kv, ld_kv, lens0, n_new, anc, ws_ml, ws_acc, B, n, Tmax, nh, Stot, s);
  cache_combine_launch(ws_acc, ws_ml, out, lse, B * n, nh, hd, Stot, s, n_new, (int)n);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_tree_accept_greedy: one wave per sequence; lane r holds row r, a ballot finds the children that match, the lowest bit wins
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void tree_accept_kernel(const int64_t* __restrict__ tok, const int32_t* __restrict__ parent,
                                                         const int32_t* __restrict__ n_new, const int64_t* __restrict__ pred,
                                                         const float* __restrict__ logp, int32_t* __restrict__ n_accept,
                                                         int32_t* __restrict__ path, int64_t* __restrict__ acc_tok, int64_t* __restrict__ next_tok,
                                                         float* __restrict__ logp_out, int n) {
  const int64_t b = blockIdx.x;
  const int r = threadIdx.x;
  const int cb = tree_clamp(n_new != nullptr ? n_new[b] : n, 0, n);
  const bool real = r >= 1 && r < cb;
  const int64_t my_tok = real ? tok[b * n + r] : 0;
  const int my_par = real ? parent[b * n + r] : -2;
  // lane d keeps entry d of every output and stores it once, after the walk: path -1, token 0 and log-probability 0 beyond the accepted depths
  int my_path = r == 0 ? 0 : -1;
  int64_t my_acc = 0;
  float my_lp = 0.f;
  int cur = 0, na = 0;
  for (int step = 1; step < n; ++step) {  // (cur, na wave-uniform)
    const int64_t want = pred[b * n + cur];
    const unsigned long long hit = __ballot(real && my_par == cur && my_tok == want);
    if (hit == 0ull) break;
    const int child = __builtin_ctzll(hit);  // the smallest-index child; child > cur, so the walk ends
    if (r == step) my_path = child;
    if (r == step - 1) {
      my_acc = want;
      my_lp = logp[b * n + cur];  // the accepted token IS row cur's prediction: its log-probability
    }
    cur = child;
    na = step;
  }
  if (r == na) my_lp = logp[b * n + cur];  // of next_tok, the prediction of the last accepted row
  if (r < n) {
    path[b * n + r] = my_path;
    logp_out[b * n + r] = my_lp;
    if (r < n - 1) acc_tok[b * (n - 1) + r] = my_acc;
  }
  if (r == 0) {
    n_accept[b] = na;
    next_tok[b] = pred[b * n + cur];
  }
}

extern "C" int plm_tree_accept_greedy(const int64_t* tok, const int32_t* parent, const int32_t* n_new, const int64_t* pred, const float* logp,
                                      int32_t* n_accept, int32_t* path, int64_t* acc_tok, int64_t* next_tok, float* logp_out, int64_t B, int64_t n,
                                      void* stream) {
  PLM_REQUIRE(tok && parent && pred && logp && n_accept && path && next_tok && logp_out && (acc_tok || n == 1), "plm_tree_accept_greedy: null pointer");
  PLM_REQUIRE(B >= 1 && B < ((int64_t)1 << 31) && n >= 1 && n <= TREE_MAX_ROWS, "plm_tree_accept_greedy: bad shape B=%ld n=%ld (need B >= 1, 1 <= n <= %d)",
              (long)B, (long)n, TREE_MAX_ROWS);
  hipLaunchKernelGGL(tree_accept_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, tok, parent, n_new, pred, logp, n_accept, path, acc_tok,
                     next_tok, logp_out, (int)n);
  PLM_CHECK_LAUNCH("plm_tree_accept_greedy");
  return PLM_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_kv_tree_commit: the accepted path's rows move to the front of the chunk, all layers in one launch through a pointer table
// ---------------------------------------------------------------------------------------------------------------------------------
struct TreeCommitTable {
  uint16_t* kv[TREE_MAX_LAYERS];
};

// A thread owns one 16-byte column chunk of one (layer, sequence) and walks d = 1 .. n_accept in ascending order: load row lens0 + path[d],
// store row lens0 + d.  No barrier is needed: path is strictly increasing with path[d] >= d (a node's index is at least its depth, as
// parent[r] < r), so every later source path[d'] >= d' > d lies beyond every row written so far - no source is overwritten before it is
// read - and two threads never touch the same columns.  A path that breaks the rule ends the walk (nothing outside the chunk's rows is
// ever addressed).  Rows beyond lens0 + n_accept stay as they are: the lengths the caller sets never reach them.
__global__ __launch_bounds__(256) void kv_tree_commit_kernel(const TreeCommitTable tab, int64_t ld_kv, const int32_t* __restrict__ lens0,
                                                             const int32_t* __restrict__ path, const int32_t* __restrict__ n_accept, int L, int B,
                                                             int n, int Tmax, int cpr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)L * B * cpr) return;
  const int c = (int)(i % cpr), b = (int)((i / cpr) % B), layer = (int)(i / ((int64_t)cpr * B));
  const int l0 = lens0[b];
  if (l0 < 0 || l0 >= Tmax) return;
  const int na = min(tree_clamp(n_accept[b], 0, n - 1), Tmax - 1 - l0);
  uint16_t* base = tab.kv[layer] + ((int64_t)b * Tmax + l0) * ld_kv + c * 8;
  int prev = 0;
  for (int d = 1; d <= na; ++d) {
    const int src = path[(int64_t)b * n + d];
    if (src <= prev || src < d || src >= n || l0 + src >= Tmax) return;
    prev = src;
    if (src != d) st_bf16x8(base + (int64_t)d * ld_kv, ld_bf16x8(base + (int64_t)src * ld_kv));
  }
}

extern "C" int plm_kv_tree_commit(uint16_t** kv_layers, int64_t n_layers, int64_t ld_kv, const int32_t* lens0, const int32_t* path,
                                  const int32_t* n_accept, int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd, void* stream) {
  const char* fn = "plm_kv_tree_commit";
  PLM_REQUIRE(kv_layers && lens0 && path && n_accept, "%s: null pointer", fn);
  PLM_REQUIRE(n_layers >= 1 && n_layers <= 65536 && n >= 1 && n <= TREE_MAX_ROWS && cache_shape_ok(B, 1, nh, hd, Tmax),
              "%s: bad shape layers=%ld B=%ld n=%ld Tmax=%ld nh=%ld hd=%ld", fn, (long)n_layers, (long)B, (long)n, (long)Tmax, (long)nh, (long)hd);
  PLM_REQUIRE(ld_kv >= 2 * nh * hd && ld_kv % 8 == 0, "%s: the cache's row stride must be a multiple of 8 and at least 2*nh*hd", fn);
  for (int64_t l = 0; l < n_layers; ++l)
    PLM_REQUIRE(kv_layers[l] && (reinterpret_cast<uintptr_t>(kv_layers[l]) & 15) == 0, "%s: layer %ld's cache is null or not 16-byte aligned", fn, (long)l);
  const int cpr = (int)(2 * nh * hd / 8);
  PLM_REQUIRE(plm_cdiv((int64_t)TREE_MAX_LAYERS * B * cpr, 256) < ((int64_t)1 << 31), "%s: bad shape: B*nh*hd too large for one launch", fn);
  for (int64_t first = 0; first < n_layers; first += TREE_MAX_LAYERS) {
    const int L = (int)(n_layers - first < TREE_MAX_LAYERS ? n_layers - first : TREE_MAX_LAYERS);
    TreeCommitTable tab{};
    for (int l = 0; l < L; ++l) tab.kv[l] = kv_layers[first + l];
    hipLaunchKernelGGL(kv_tree_commit_kernel, dim3((unsigned)plm_cdiv((int64_t)L * B * cpr, 256)), dim3(256), 0, (hipStream_t)stream, tab, ld_kv, lens0,
                       path, n_accept, L, (int)B, (int)n, (int)Tmax, cpr);
    PLM_CHECK_LAUNCH(fn);
  }
  return PLM_OK;
}
