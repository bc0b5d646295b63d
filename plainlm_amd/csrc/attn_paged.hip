// The paged KV cache for gfx950: the cached step of attn_cache.hip over a pool of fixed-size pages behind a block
// table, so that cache memory follows the tokens that exist and a sequence joins or leaves a batch by editing a few int32 words.
//
// Pool: pool[n_pages, PLM_KV_PAGE_ROWS, ld_kv] bf16 per layer, every row the k | v columns of attn_cache.hip's cache row (k rotated).
// Table: table[B, max_pages] int32, entry (b, i) = the page that holds tokens 64*i .. 64*i + 63 of sequence b, -1 for none.  The row of
// token j of sequence b is pool + (table[b, j / 64] * 64 + j % 64) * ld_kv.
//
// kv_paged_append_rope_rows_kernel is kv_append_rope_rows_kernel (same table loads, same rope8, so the same bits) with that address and
// the page checks added to its refusal predicate; kv_paged_store_rows_kernel scatters a prompt's rotated k | v rows (prefill).
//
// attn_decode_paged_kernel (one query row per sequence) splits by LENGTH: a workgroup owns one (sequence, head, chunk) of
// PLM_KV_PAGED_CHUNK keys, sequence b has ceil(lens[b] / chunk) live chunks, and a workgroup whose chunk starts at or beyond lens[b]
// writes the empty partial and leaves.  Its chunk's page ids (at most chunk / 64) go to LDS once; inside the key loop a wave's
// DEC_UNROLL * KPW rows lie in one page (64 is a multiple of the 16 / 32 / 64 rows a wave has in flight at hd 128 / 64 / 32), so the page
// id is one wave-uniform LDS read made scalar, the page's base one scalar address, and what a lane adds to it - (row in the group) *
// ld_kv + its column - is computed once before the loop.  No lane reads the table in the loop.  Everything after the loads is
// attn_decode_split_kernel's arithmetic in its order: hd / 8 lanes per key row, 16-byte loads all issued first, the base-2 online
// softmax in fp32, lane groups -> wave -> workgroup in fixed order, partials (m, l, acc[hd]) in the layout cache_combine_launch reads.
// No atomics.  A sequence's bits depend on its own length and rows alone: not on B, not on the other sequences, not on Lcap (an empty
// partial is skipped by the combine) and not on where its pages lie.
//
// attn_extend_paged_kernel (n query rows per sequence, causal inside the chunk) keeps attn_extend_kernel's body - GenTile K / V tiles in
// LDS, S^T = K Q^T on MFMA, the `lim` ballot, tile loads clamped to the last valid row - with the split ranges ALIGNED TO PAGES: a split
// is ceil(ceil(L / 64) / S) whole pages, so every 64-key tile lies in one page and is fetched from table[b, kv0 / 64] with one
// workgroup-uniform table read per tile.
//
// A table entry outside [0, n_pages) is never turned into an address: the append refuses the sequence (status[0] = 1), the attention
// kernels skip that page's keys.
#include "attn_gen_tile.h"
#include "attn_cache.h"

#include "../../include/plainlm_hip.h"

#ifndef PLM_KV_PAGED_CHUNK
#define PLM_KV_PAGED_CHUNK 512  // keys per decode workgroup: the fastest of 128 / 256 / 512 in profiles/paged_bench.txt
#endif
static_assert(PLM_KV_PAGED_CHUNK % PLM_KV_PAGE_ROWS == 0 && PLM_KV_PAGED_CHUNK >= 128 && PLM_KV_PAGED_CHUNK <= 512, "chunk: 128 .. 512, whole pages");
static_assert(PLM_KV_PAGE_ROWS == 64, "the page is attn_extend_paged_kernel's key tile");

#define PG_ROWS PLM_KV_PAGE_ROWS
#define PG_CHUNK PLM_KV_PAGED_CHUNK
#define PG_CHUNK_PAGES (PG_CHUNK / PG_ROWS)
#define PG_THREADS 256
#define PG_WAVES (PG_THREADS / PLM_WAVE)
#define PG_UNROLL 4

__device__ __forceinline__ int pg_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ bool pg_page_ok(int page, int n_pages) { return (unsigned)page < (unsigned)n_pages; }
// exp2(x - m) without the -inf - -inf of a softmax that has seen nothing yet (attn_cache.hip's dec_base)
__device__ __forceinline__ float pg_base(float m) { return m == -INFINITY ? 0.f : m; }

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_kv_paged_append_rope_rows: one thread per 16-byte chunk of a qkv row
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kv_paged_append_rope_rows_kernel(const uint16_t* __restrict__ qkv, int64_t ld_qkv,
                                                                        const int32_t* __restrict__ lens0, const int32_t* __restrict__ n_new,
                                                                        const float* __restrict__ rcos, const float* __restrict__ rsin,
                                                                        int rope_T, uint16_t* __restrict__ q_out, uint16_t* __restrict__ pool,
                                                                        int64_t ld_kv, const int32_t* __restrict__ table,
                                                                        int32_t* __restrict__ status, int B, int n, int max_pages, int n_pages,
                                                                        int nh, int hd) {
  const int dm = nh * hd;
  const int cpr = 3 * dm / 8;  // 16-byte chunks per qkv row
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * n * cpr) return;
  const int64_t row = i / cpr;  // b * n + r
  const int c = (int)(i - row * cpr);
  const int b = (int)(row / n), r = (int)(row - (int64_t)b * n);
  const int col = c * 8;
  const int l0 = lens0[b];
  const int cb = pg_clamp(n_new != nullptr ? n_new[b] : n, 0, n);
  // kv_append_rope_rows_kernel's predicate with Tmax = max_pages * 64 ...
  bool refused = l0 < 0 || (int64_t)l0 + cb > (int64_t)max_pages * PG_ROWS || (int64_t)l0 + cb > rope_T;
  // ... extended by the pages: every page the chunk's rows l0 .. l0 + cb - 1 lie in must be a page of the pool
  if (!refused && cb > 0) {
    const int32_t* trow = table + (int64_t)b * max_pages;
    for (int pi = l0 / PG_ROWS; pi <= (l0 + cb - 1) / PG_ROWS; ++pi) refused = refused || !pg_page_ok(trow[pi], n_pages);
  }
  if (refused && r == 0 && c == 0) status[0] = 1;
  if (refused || r >= cb) {  // no cache row: a q row of zeros
    if (col < dm) st_bf16x8(q_out + row * dm + col, zero_bf16x8());
    return;
  }
  const int t = l0 + r;
  bf16x8_t v = ld_bf16x8(qkv + row * ld_qkv + col);
  if (col < 2 * dm) {  // q | k: the rotation of rope_qk_kernel (attn.hip), same table loads, same rope8
    const int pair0 = (col % hd) / 2;
    const f32x4_t cs = *reinterpret_cast<const f32x4_t*>(rcos + (int64_t)t * (hd / 2) + pair0);
    const f32x4_t sn = *reinterpret_cast<const f32x4_t*>(rsin + (int64_t)t * (hd / 2) + pair0);
    v = rope8(v, cs, sn, 1.f);
  }
  if (col < dm) {
    st_bf16x8(q_out + row * dm + col, v);
  } else {
    const int page = table[(int64_t)b * max_pages + t / PG_ROWS];
    st_bf16x8(pool + ((int64_t)page * PG_ROWS + t % PG_ROWS) * ld_kv + (col - dm), v);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_kv_paged_store_rows: rows [B, T, ld_rows] (k | v, 2 * dm wide) -> the pages of rows t < lens[b]; one thread per 16 bytes
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kv_paged_store_rows_kernel(const uint16_t* __restrict__ rows, int64_t ld_rows,
                                                                  const int32_t* __restrict__ lens, uint16_t* __restrict__ pool,
                                                                  int64_t ld_kv, const int32_t* __restrict__ table,
                                                                  int32_t* __restrict__ status, int B, int T, int max_pages, int n_pages,
                                                                  int dm) {
  const int cpr = 2 * dm / 8;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T * cpr) return;
  const int64_t row = i / cpr;  // b * T + t
  const int c = (int)(i - row * cpr);
  const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
  if (t >= lens[b]) return;  // padding: no page is asked for, nothing is written
  const int page = t / PG_ROWS < max_pages ? table[(int64_t)b * max_pages + t / PG_ROWS] : -1;
  if (!pg_page_ok(page, n_pages)) {  // a row without a page is not stored
    if (c == 0) status[0] = 1;
    return;
  }
  st_bf16x8(pool + ((int64_t)page * PG_ROWS + t % PG_ROWS) * ld_kv + c * 8, ld_bf16x8(rows + row * ld_rows + c * 8));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_attn_decode_paged
// ---------------------------------------------------------------------------------------------------------------------------------
// grid (B*nh, NC), NC = ceil(Lcap / PG_CHUNK); partial (bh, c) at index bh * NC + c of ws_ml [., 2] / ws_acc [., hd]
template <int HD>
__global__ __launch_bounds__(PG_THREADS) void attn_decode_paged_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ pool,
                                                                       int64_t ld_kv, const int32_t* __restrict__ table,
                                                                       const int32_t* __restrict__ lens, float* __restrict__ ws_ml,
                                                                       float* __restrict__ ws_acc, int Lcap, int max_pages, int n_pages, int nh,
                                                                       float c2) {
  constexpr int G = HD / 8;            // lanes per key row
  constexpr int KPW = PLM_WAVE / G;    // key rows per wave and load instruction
  constexpr int RPW = KPW * PG_UNROLL; // key rows a wave has in flight: 16 / 32 / 64, a divisor of the page
  static_assert(PG_ROWS % RPW == 0, "a wave's rows in flight must not straddle a page");
  __shared__ int s_page[PG_CHUNK_PAGES];
  __shared__ float s_ml[PG_WAVES][2];
  __shared__ float s_acc[PG_WAVES][HD];

  const int bh = blockIdx.x, ck = blockIdx.y, NC = gridDim.y;
  const int b = bh / nh, h = bh - b * nh;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid / PLM_WAVE), lane = tid % PLM_WAVE;
  const int grp = lane / G, sub = lane % G;
  const int dm = nh * HD;
  const int64_t part = (int64_t)bh * NC + ck;

  const int len = pg_clamp(lens[b], 0, Lcap);
  const int k0 = ck * PG_CHUNK;
  if (k0 >= len) {  // not a chunk of this sequence: the empty partial, nothing else is read
    if (tid < HD) ws_acc[part * HD + tid] = 0.f;
    if (tid == 0) {
      ws_ml[part * 2] = -INFINITY;
      ws_ml[part * 2 + 1] = 0.f;
    }
    return;
  }
  const int nk = min(PG_CHUNK, len - k0);  // keys of this chunk
  // the chunk's page ids, once; an entry that is no page of the pool is kept as -1 and its keys are skipped
  if (tid < PG_CHUNK_PAGES) {
    int pg = -1;
    if (tid * PG_ROWS < nk) pg = table[(int64_t)b * max_pages + k0 / PG_ROWS + tid];  // k0 + nk <= Lcap <= max_pages * 64
    s_page[tid] = pg_page_ok(pg, n_pages) ? pg : -1;
  }

  // q slice of this lane, pre-scaled to log2 units
  float qf[8];
  {
    const bf16x8_t qv = ld_bf16x8(q + (int64_t)b * dm + h * HD + sub * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[e] = bf2f(qv[e]) * c2;
  }
  // what this lane adds to a wave's row base, for each of its rows in flight: fixed for the whole loop
  int64_t loff[PG_UNROLL];
#pragma unroll
  for (int u = 0; u < PG_UNROLL; ++u) loff[u] = (int64_t)(u * KPW + grp) * ld_kv + h * HD + sub * 8;
  __syncthreads();

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;

  for (int j0 = wave * RPW; j0 < nk; j0 += PG_WAVES * RPW) {  // j0: offset inside the chunk, wave-uniform
    const int page = __builtin_amdgcn_readfirstlane(s_page[j0 / PG_ROWS]);
    if (page < 0) continue;
    const uint16_t* base = pool + ((int64_t)page * PG_ROWS + j0 % PG_ROWS) * ld_kv;  // scalar: row j0 of the chunk, column 0
    bf16x8_t kk[PG_UNROLL], vv[PG_UNROLL];
    bool ok[PG_UNROLL];
#pragma unroll
    for (int u = 0; u < PG_UNROLL; ++u) {  // all loads first: the kernel lives on memory-level parallelism
      ok[u] = j0 + u * KPW + grp < nk;     // rows at and beyond lens[b] are never read (they may hold anything)
      kk[u] = zero_bf16x8();
      vv[u] = zero_bf16x8();
      if (ok[u]) {
        kk[u] = ld_bf16x8(base + loff[u]);
        vv[u] = ld_bf16x8(base + loff[u] + dm);
      }
    }
#pragma unroll
    for (int u = 0; u < PG_UNROLL; ++u) {
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d = fmaf(qf[e], bf2f(kk[u][e]), d);
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, PLM_WAVE);  // inside the lane group
      const float sc = ok[u] ? d : -INFINITY;
      const float mn = fmaxf(m, sc);
      const float bs = pg_base(mn);
      const float alpha = __builtin_amdgcn_exp2f(m - bs);
      const float p = __builtin_amdgcn_exp2f(sc - bs);
      l = l * alpha + p;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = acc[e] * alpha + p * bf2f(vv[u][e]);
      m = mn;
    }
  }

  // lane groups of a wave -> one partial (butterfly over the group index: every group ends with the same value)
#pragma unroll
  for (int o = G; o < PLM_WAVE; o <<= 1) {
    const float m2 = __shfl_xor(m, o, PLM_WAVE), l2 = __shfl_xor(l, o, PLM_WAVE);
    const float mn = fmaxf(m, m2), bs = pg_base(mn);
    const float a = __builtin_amdgcn_exp2f(m - bs), a2 = __builtin_amdgcn_exp2f(m2 - bs);
    l = l * a + l2 * a2;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = acc[e] * a + __shfl_xor(acc[e], o, PLM_WAVE) * a2;
    m = mn;
  }
  if (grp == 0) {
    if (sub == 0) {
      s_ml[wave][0] = m;
      s_ml[wave][1] = l;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) s_acc[wave][sub * 8 + e] = acc[e];
  }
  __syncthreads();
  // waves -> the chunk's partial, in wave order
  if (tid < HD) {
    float mm = s_ml[0][0];
#pragma unroll
    for (int w = 1; w < PG_WAVES; ++w) mm = fmaxf(mm, s_ml[w][0]);
    const float bs = pg_base(mm);
    float ll = 0.f, a = 0.f;
#pragma unroll
    for (int w = 0; w < PG_WAVES; ++w) {
      const float sc = __builtin_amdgcn_exp2f(s_ml[w][0] - bs);
      ll += s_ml[w][1] * sc;
      a += s_acc[w][tid] * sc;
    }
    if (tid == 0) {
      ws_ml[part * 2] = mm;
      ws_ml[part * 2 + 1] = ll;
    }
    ws_acc[part * HD + tid] = a;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_attn_extend_paged
// ---------------------------------------------------------------------------------------------------------------------------------
// attn_extend_kernel's workspace: acc fp32 [B*nh, S, n, hd] then ml fp32 [B*nh, S, n, 2]; rows r >= c_b are neither written nor read.
template <int HD>
__global__ __launch_bounds__(256, 2) void attn_extend_paged_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ pool,
                                                                   int64_t ld_kv, const int32_t* __restrict__ table,
                                                                   const int32_t* __restrict__ lens0, const int32_t* __restrict__ n_new,
                                                                   uint16_t* __restrict__ out, float* __restrict__ lse,
                                                                   float* __restrict__ ws_acc, float* __restrict__ ws_ml, int n, int Lcap,
                                                                   int max_pages, int n_pages, int nh, int nqt, int S, float scale) {
  using TL = GenTile<HD>;
  __shared__ __attribute__((aligned(16))) char smem[2 * TL::BYTES];  // K | V
  constexpr int NKS = HD / 16, NDB = HD / 32;
  const int qt = (int)(blockIdx.x % nqt), bh = (int)(blockIdx.x / nqt), h = bh % nh, b = bh / nh, sp = blockIdx.y;
  const int dm = nh * HD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;

  const int l0 = pg_clamp(lens0[b], 0, Lcap);
  const int cb = pg_clamp(n_new != nullptr ? n_new[b] : n, 0, n);
  const int L = (int)min((int64_t)l0 + cb, (int64_t)Lcap);  // keys of the sequence; rows at and beyond L are never loaded
  // a split is whole pages: k0 is a multiple of 64 (or L, an empty split), so a 64-key tile never straddles a page
  const int chunk = ((L + PG_ROWS - 1) / PG_ROWS + S - 1) / S * PG_ROWS;
  const int k0 = min(sp * chunk, L), k1 = min(k0 + chunk, L);

  const int q0 = qt * 128, r = q0 + wave * 32 + l31;
  const bool valid = r < cb;
  // the last key this lane's query may see inside the split (min(r, Lcap): no overflow for a huge n); -1: none
  const int lim = valid ? min(min(l0 + min(r, Lcap), Lcap - 1), k1 - 1) : -1;
  // the workgroup walks the split up to the last key its last valid row sees
  const int rlast = min(q0 + 127, cb - 1);
  const int kend = rlast < q0 ? k0 : min(k1, min(l0 + min(rlast, Lcap), Lcap - 1) + 1);

  const int32_t* trow = table + (int64_t)b * max_pages;
  const float c2 = scale * GLOG2E;
  bf16x8_t qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks)
    qf[ks] = valid ? ld_bf16x8(q + ((int64_t)b * n + r) * dm + h * HD + ks * 16 + hi * 8) : zero_bf16x8();
  f32x16_t o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) gzero16(o[db]);
  float m = -INFINITY, lsum = 0.f;
  char* sK = smem;
  char* sV = smem + TL::BYTES;
  for (int kv0 = k0; kv0 < kend; kv0 += PG_ROWS) {  // (bounds uniform over the workgroup; kv0 / 64 < ceil(L / 64) <= max_pages)
    const int page = trow[kv0 / PG_ROWS];            // uniform over the workgroup: one table read per tile
    if (!pg_page_ok(page, n_pages)) continue;        // no page of the pool: its keys are skipped, nothing is addressed
    const uint16_t* kbase = pool + (int64_t)page * PG_ROWS * ld_kv + h * HD;  // + j * ld_kv: k of the page's row j; + dm: its v
    __syncthreads();                                 // everyone is done with the previous tile
    // clamped to the sequence's last valid row inside the page: a stale row (it may hold NaN) never reaches LDS
    TL::load(sK, kbase, ld_kv, 0, min(PG_ROWS - 1, L - 1 - kv0), tid);
    TL::load(sV, kbase + dm, ld_kv, 0, min(PG_ROWS - 1, L - 1 - kv0), tid);
    __syncthreads();
    if (__ballot(kv0 <= lim) == 0) continue;            // none of this wave's 32 queries sees the tile (wave-uniform)
    const bool whole = __ballot(kv0 + 63 > lim) == 0;   // every query of the wave sees every key of it: the unmasked path
    f32x16_t s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      gzero16(s[kb]);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) s[kb] = mfma32(TL::rows(sK, kb * 32 + l31, ks, hi), qf[ks], s[kb]);
    }
    if (!whole) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (kv0 + kb * 32 + mfma32_row(e, hi) > lim) s[kb][e] = -INFINITY;
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int e = 0; e < 16; ++e) tmax = fmaxf(tmax, s[kb][e]);
    {
      float t_lo, t_hi;
      half_pair(tmax, t_lo, t_hi);
      tmax = fmaxf(t_lo, t_hi);
    }
    const float m_new = fmaxf(m, tmax * c2);
    const float m_safe = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m - m_safe);  // m = -inf: 0
    float psum = 0.f;
    bf16x8_t pf[4];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][e], c2, -m_safe));
        psum += p;
        pf[kb * 2 + (e >> 3)][e & 7] = f2bf(p);
      }
    lsum = lsum * alpha + psum;
    m = m_new;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
#pragma unroll
      for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
#pragma unroll
      for (int u = 0; u < 4; ++u) o[db] = mfma32(TL::cols(sV, db, (u >> 1) * 32 + (u & 1) * 16 + 4 * hi, lane), pf[u], o[db]);
    }
  }
  float l_lo, l_hi;
  half_pair(lsum, l_lo, l_hi);
  const float ltot = l_lo + l_hi;
  if (r >= n) return;  // past the chunk: no row of any buffer
  if (S == 1) {
    // a row at or beyond c_b saw no key: out = 0, LSE = +inf (a row that sees a key sums at least the 1 of its maximum)
    const bool empty = !(ltot > 0.f);
    const float inv = empty ? 0.f : 1.f / ltot;
    if (lse != nullptr && hi == 0) lse[(int64_t)bh * n + r] = empty ? INFINITY : m + __builtin_amdgcn_logf(ltot);  // base-2 LSE
    uint16_t* orow = out + ((int64_t)b * n + r) * dm + h * HD;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = f2bf(o[db][4 * g + e] * inv);
        st_bf16x4(orow + db * 32 + 8 * g + 4 * hi, v);
      }
  } else if (valid) {
    const int64_t part = ((int64_t)bh * S + sp) * n + r;  // an empty split: (m = -inf, l = 0, acc = 0)
    if (hi == 0) {
      ws_ml[part * 2] = m;
      ws_ml[part * 2 + 1] = ltot;
    }
    float* arow = ws_acc + part * HD;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = o[db][4 * g + e];
        *reinterpret_cast<f32x4_t*>(arow + db * 32 + 8 * g + 4 * hi) = v;
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int plm_kv_page_rows(void) { return PG_ROWS; }
extern "C" int plm_kv_paged_chunk_rows(void) { return PG_CHUNK; }

// what every entry point here asks of the pool and the table
static int paged_check_pool(const char* fn, const void* pool, int64_t ld_kv, const void* table, int64_t max_pages, int64_t n_pages, int64_t nh,
                            int64_t hd) {
  PLM_REQUIRE(pool && table, "%s: null pointer", fn);
  PLM_REQUIRE(hd == 32 || hd == 64 || hd == 128, "%s: head_dim %ld unsupported (32, 64, 128)", fn, (long)hd);
  PLM_REQUIRE(nh > 0 && nh < 65536 && max_pages > 0 && max_pages < (1 << 18) && n_pages > 0 && n_pages < (1 << 24),
              "%s: bad shape nh=%ld max_pages=%ld n_pages=%ld (max_pages < 2^18, n_pages < 2^24)", fn, (long)nh, (long)max_pages, (long)n_pages);
  PLM_REQUIRE(ld_kv >= 2 * nh * hd && ld_kv % 8 == 0, "%s: the pool's row stride must be a multiple of 8 and at least 2*nh*hd", fn);
  PLM_REQUIRE((reinterpret_cast<uintptr_t>(pool) & 15) == 0 && (reinterpret_cast<uintptr_t>(table) & 3) == 0,
              "%s: the pool must be 16-byte aligned, the table 4-byte aligned", fn);
  return PLM_OK;
}

extern "C" int plm_kv_paged_append_rope_rows(const uint16_t* qkv, int64_t ld_qkv, const int32_t* lens0, const int32_t* n_new,
                                             const float* rope_cos, const float* rope_sin, int64_t rope_T, uint16_t* q_out, uint16_t* pool,
                                             int64_t ld_kv, const int32_t* table, int32_t* status, int64_t B, int64_t n, int64_t max_pages,
                                             int64_t n_pages, int64_t nh, int64_t hd, void* stream) {
  const char* fn = "plm_kv_paged_append_rope_rows";
  PLM_REQUIRE(qkv && lens0 && rope_cos && rope_sin && q_out && status, "%s: null pointer", fn);
  if (const int e = paged_check_pool(fn, pool, ld_kv, table, max_pages, n_pages, nh, hd)) return e;
  PLM_REQUIRE(cache_shape_ok(B, n, nh, hd, max_pages * PG_ROWS) && rope_T > 0 && rope_T < (1 << 24),
              "%s: bad shape B=%ld n=%ld max_pages=%ld nh=%ld rope_T=%ld (n >= 1, B*n < 2^31)", fn, (long)B, (long)n, (long)max_pages, (long)nh,
              (long)rope_T);
  PLM_REQUIRE(ld_qkv >= 3 * nh * hd && ld_qkv % 8 == 0, "%s: the qkv row stride must be a multiple of 8 and at least 3*nh*hd", fn);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(q_out) | reinterpret_cast<uintptr_t>(rope_cos) |
                reinterpret_cast<uintptr_t>(rope_sin)) & 15) == 0,
              "%s: qkv, q_out and the RoPE tables must be 16-byte aligned", fn);
  const int64_t blocks = plm_cdiv(B * n * (3 * nh * hd / 8), 256);
  PLM_REQUIRE(blocks < ((int64_t)1 << 31), "%s: bad shape: B*n*nh*hd too large for one launch", fn);
  hipLaunchKernelGGL(kv_paged_append_rope_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, qkv, ld_qkv, lens0, n_new,
                     rope_cos, rope_sin, (int)rope_T, q_out, pool, ld_kv, table, status, (int)B, (int)n, (int)max_pages, (int)n_pages, (int)nh,
                     (int)hd);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" int plm_kv_paged_store_rows(const uint16_t* rows, int64_t ld_rows, const int32_t* lens, uint16_t* pool, int64_t ld_kv,
                                       const int32_t* table, int32_t* status, int64_t B, int64_t T, int64_t max_pages, int64_t n_pages,
                                       int64_t nh, int64_t hd, void* stream) {
  const char* fn = "plm_kv_paged_store_rows";
  PLM_REQUIRE(rows && lens && status, "%s: null pointer", fn);
  if (const int e = paged_check_pool(fn, pool, ld_kv, table, max_pages, n_pages, nh, hd)) return e;
  PLM_REQUIRE(cache_shape_ok(B, T, nh, hd, max_pages * PG_ROWS), "%s: bad shape B=%ld T=%ld max_pages=%ld nh=%ld (T >= 1, B*T < 2^31)", fn, (long)B,
              (long)T, (long)max_pages, (long)nh);
  PLM_REQUIRE(ld_rows >= 2 * nh * hd && ld_rows % 8 == 0, "%s: the rows' stride must be a multiple of 8 and at least 2*nh*hd", fn);
  PLM_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 15) == 0, "%s: rows must be 16-byte aligned", fn);
  const int64_t blocks = plm_cdiv(B * T * (2 * nh * hd / 8), 256);
  PLM_REQUIRE(blocks < ((int64_t)1 << 31), "%s: bad shape: B*T*nh*hd too large for one launch", fn);
  hipLaunchKernelGGL(kv_paged_store_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, rows, ld_rows, lens, pool, ld_kv,
                     table, status, (int)B, (int)T, (int)max_pages, (int)n_pages, (int)(nh * hd));
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

// the attention entry points' shared refusals; Lcap: the keys of the table the caller wants walked
static int paged_check_attend(const char* fn, const uint16_t* q, const uint16_t* pool, int64_t ld_kv, const int32_t* table, const int32_t* lens,
                              const uint16_t* out, int64_t B, int64_t n, int64_t Lcap, int64_t max_pages, int64_t n_pages, int64_t nh, int64_t hd,
                              const void* workspace) {
  PLM_REQUIRE(q && lens && out && workspace, "%s: null pointer", fn);
  if (const int e = paged_check_pool(fn, pool, ld_kv, table, max_pages, n_pages, nh, hd)) return e;
  PLM_REQUIRE(cache_shape_ok(B, n, nh, hd, max_pages * PG_ROWS) && Lcap >= 1 && Lcap <= max_pages * PG_ROWS,
              "%s: bad shape B=%ld n=%ld Lcap=%ld max_pages=%ld nh=%ld (n >= 1, B*n < 2^31, 1 <= Lcap <= max_pages * %d)", fn, (long)B, (long)n,
              (long)Lcap, (long)max_pages, (long)nh, PG_ROWS);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
              "%s: q, out and the workspace must be 16-byte aligned", fn);
  return PLM_OK;
}

extern "C" size_t plm_attn_decode_paged_workspace_bytes(int64_t B, int64_t nh, int64_t hd, int64_t Lcap) {
  if (!cache_shape_ok(B, 1, nh, hd, Lcap) || plm_cdiv(Lcap, PG_CHUNK) > CACHE_MAX_SPLITS) return 0;
  return cache_ws_bytes(B, 1, nh, hd, (int)plm_cdiv(Lcap, PG_CHUNK));
}

template <int HD>
static void paged_dec_launch(const uint16_t* q, const uint16_t* pool, int64_t ld_kv, const int32_t* table, const int32_t* lens, uint16_t* out,
                             float* lse, int64_t B, int64_t Lcap, int64_t max_pages, int64_t n_pages, int64_t nh, int NC, float* ws, hipStream_t s) {
  float* ws_ml = ws;
  float* ws_acc = ws + (size_t)B * nh * NC * 2;
  const float c2 = (1.f / sqrtf((float)HD)) * GLOG2E;
  hipLaunchKernelGGL(attn_decode_paged_kernel<HD>, dim3((unsigned)(B * nh), (unsigned)NC), dim3(PG_THREADS), 0, s, q, pool, ld_kv, table, lens,
                     ws_ml, ws_acc, (int)Lcap, (int)max_pages, (int)n_pages, (int)nh, c2);
  cache_combine_launch(ws_acc, ws_ml, out, lse, B, nh, HD, NC, s);
}

extern "C" int plm_attn_decode_paged(const uint16_t* q, const uint16_t* pool, int64_t ld_kv, const int32_t* table, const int32_t* lens,
                                     uint16_t* out, float* lse, int64_t B, int64_t Lcap, int64_t max_pages, int64_t n_pages, int64_t nh,
                                     int64_t hd, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "plm_attn_decode_paged";
  if (const int e = paged_check_attend(fn, q, pool, ld_kv, table, lens, out, B, 1, Lcap, max_pages, n_pages, nh, hd, workspace)) return e;
  const int64_t NC = plm_cdiv(Lcap, PG_CHUNK);
  PLM_REQUIRE(NC <= CACHE_MAX_SPLITS, "%s: Lcap=%ld is %ld chunks of %d keys, more than %d (walk fewer keys per call)", fn, (long)Lcap, (long)NC,
              PG_CHUNK, CACHE_MAX_SPLITS);
  const size_t need = cache_ws_bytes(B, 1, nh, hd, (int)NC);
  if (workspace_bytes < need) {
    plm_set_error("%s: workspace of %zu bytes required, %zu given", fn, need, workspace_bytes);
    return PLM_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  if (hd == 32) paged_dec_launch<32>(q, pool, ld_kv, table, lens, out, lse, B, Lcap, max_pages, n_pages, nh, (int)NC, ws, s);
  else if (hd == 64) paged_dec_launch<64>(q, pool, ld_kv, table, lens, out, lse, B, Lcap, max_pages, n_pages, nh, (int)NC, ws, s);
  else paged_dec_launch<128>(q, pool, ld_kv, table, lens, out, lse, B, Lcap, max_pages, n_pages, nh, (int)NC, ws, s);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" size_t plm_attn_extend_paged_workspace_bytes(int64_t B, int64_t n, int64_t nh, int64_t hd, int64_t Lcap, int splits) {
  if (!cache_shape_ok(B, n, nh, hd, Lcap) || splits < 0 || splits > CACHE_MAX_SPLITS) return 0;
  return cache_ws_bytes(B, n, nh, hd, cache_resolve_splits(B, n, nh, Lcap, splits));
}

template <int HD>
static void paged_ext_launch(const uint16_t* q, const uint16_t* pool, int64_t ld_kv, const int32_t* table, const int32_t* lens0,
                             const int32_t* n_new, uint16_t* out, float* lse, int64_t B, int64_t n, int64_t Lcap, int64_t max_pages,
                             int64_t n_pages, int64_t nh, int S, float* ws, hipStream_t s) {
  float* ws_acc = ws;
  float* ws_ml = ws + (size_t)B * nh * S * n * HD;
  const int nqt = (int)plm_cdiv(n, 128);
  const float scale = 1.f / sqrtf((float)HD);
  hipLaunchKernelGGL(attn_extend_paged_kernel<HD>, dim3((unsigned)(B * nh * nqt), (unsigned)S), dim3(256), 0, s, q, pool, ld_kv, table, lens0,
                     n_new, out, lse, ws_acc, ws_ml, (int)n, (int)Lcap, (int)max_pages, (int)n_pages, (int)nh, nqt, S, scale);
  if (S > 1) cache_combine_launch(ws_acc, ws_ml, out, lse, B, nh, HD, S, s, n_new, 0, n);  // attn_cache_combine_kernel's chunk form
}

extern "C" int plm_attn_extend_paged(const uint16_t* q, const uint16_t* pool, int64_t ld_kv, const int32_t* table, const int32_t* lens0,
                                     const int32_t* n_new, uint16_t* out, float* lse, int64_t B, int64_t n, int64_t Lcap, int64_t max_pages,
                                     int64_t n_pages, int64_t nh, int64_t hd, int splits, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  const char* fn = "plm_attn_extend_paged";
  if (const int e = paged_check_attend(fn, q, pool, ld_kv, table, lens0, out, B, n, Lcap, max_pages, n_pages, nh, hd, workspace)) return e;
  PLM_REQUIRE(splits >= 0 && splits <= CACHE_MAX_SPLITS, "%s: splits=%d out of range (0 = automatic, 1..%d forced)", fn, splits, CACHE_MAX_SPLITS);
  PLM_REQUIRE(B * n * nh * plm_cdiv(n, 128) < ((int64_t)1 << 31), "%s: bad shape: B*n*nh too large for one launch", fn);
  const int S = cache_resolve_splits(B, n, nh, Lcap, splits);
  const size_t need = cache_ws_bytes(B, n, nh, hd, S);
  if (workspace_bytes < need) {
    plm_set_error("%s: workspace of %zu bytes required, %zu given", fn, need, workspace_bytes);
    return PLM_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  if (hd == 32) paged_ext_launch<32>(q, pool, ld_kv, table, lens0, n_new, out, lse, B, n, Lcap, max_pages, n_pages, nh, S, ws, s);
  else if (hd == 64) paged_ext_launch<64>(q, pool, ld_kv, table, lens0, n_new, out, lse, B, n, Lcap, max_pages, n_pages, nh, S, ws, s);
  else paged_ext_launch<128>(q, pool, ld_kv, table, lens0, n_new, out, lse, B, n, Lcap, max_pages, n_pages, nh, S, ws, s);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}
