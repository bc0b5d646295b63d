// The cached step for gfx950 (DESIGN.md sections 12 and 14): append n rotated tokens per sequence to the per-layer KV cache, and attend
// the n new query rows per sequence over that cache.  n = 1 is a decode step (plm_kv_append_rope, plm_attn_decode), n >= 1 a cache
// extension (plm_kv_append_rope_rows, plm_attn_extend).  The append kernel, the combine kernel, the split rule, the shape limits and the
// argument checks are written once; the two attention kernels are two designs and stay two kernels.
//
// Cache: kv[B, Tmax, ld_kv] bf16, row (b, j) = the k | v column blocks (2 * nh * hd values) of token j of sequence b, k already rotated -
// the bits plm_qkv_rope_bf16 leaves in columns [nh*hd, 3*nh*hd) of its output.  Nothing is transposed.
//
// Both attention kernels split the keys of a sequence into S contiguous ranges of ceil(L / S) keys (flash-decoding), leave fp32 partials
// (m, l, acc[hd]) per (query row, split) in the workspace, and the combine walks them in split order.  No atomics: every partial is
// written by one workgroup, so the result is bit-reproducible and, for a fixed split count, independent of what the other sequences hold.
//
// attn_decode_split_kernel (one query row) is a bandwidth problem (one q row against lens[b] rows of 2 * hd * 2 bytes per head), so there
// is no MFMA in it: a group of hd / 8 lanes owns one key row, every lane loads 16 bytes of k and 16 bytes of v, the dot product is 8 VALU
// FMAs plus a butterfly inside the group, and the softmax is an online base-2 softmax in fp32 (P is never rounded to bf16).
//
// attn_extend_kernel (a chunk of n query rows, causal inside the chunk, at per-sequence offsets) is attn_fwd_masked_kernel
// (attn_masked.hip) with the packed mask word replaced by arithmetic: 64-key K / V tiles copied to LDS by the whole workgroup
// (GenTile<HD>), 32 query rows per wave, S^T = K Q^T so a lane owns a query, fp32 statistics, bf16 P, the m_safe guard.  Query row r of
// sequence b (r < c_b) sees key j iff j <= lens0[b] + r; every lane carries that as ONE number, `lim` (the last key it may see inside this
// split's range, -1 for a row past c_b), so a tile is skipped, masked or taken whole by a ballot of one comparison.  Tile loads are
// clamped to the sequence's last valid row lens0[b] + c_b - 1: a stale cache row may hold NaN, a masked score gives P = 0, and 0 * NaN in
// the P V product is NaN - such a row must never reach LDS.  Its grid is (B*nh*ceil(n/128)) x S; S == 1 writes out directly (one launch).
// With n <= 32 only wave 0 of a workgroup holds query rows: the four waves load the tiles together and one computes; the parallelism of
// a short chunk comes from the splits, as in the decode kernel.
#include "attn_gen_tile.h"

#include "../../include/plainlm_hip.h"

#define DEC_THREADS 256
#define DEC_WAVES (DEC_THREADS / PLM_WAVE)
#define DEC_UNROLL 4
#define CACHE_MAX_SPLITS 64
// the automatic split rule knows the device by this one number (MI355X: 256 CUs); nothing is queried, nothing is read back
#define CACHE_CUS 256

__device__ __forceinline__ int ext_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_kv_append_rope (n = 1, n_new = NULL, lens0 = pos) and plm_kv_append_rope_rows: one thread per 16-byte chunk of a qkv row
// ---------------------------------------------------------------------------------------------------------------------------------
// zero_q: a row without a cache row (refused sequence, or r >= c_b) still gets a defined q_out row (the rows contract); without it such
// a row writes nothing at all (the decode contract: q_out stays as the caller left it).
__global__ __launch_bounds__(256) void kv_append_rope_rows_kernel(const uint16_t* __restrict__ qkv, int64_t ld_qkv,
                                                                  const int32_t* __restrict__ lens0, const int32_t* __restrict__ n_new,
                                                                  const float* __restrict__ rcos, const float* __restrict__ rsin, int rope_T,
                                                                  uint16_t* __restrict__ q_out, uint16_t* __restrict__ kv, int64_t ld_kv,
                                                                  int32_t* __restrict__ status, int B, int n, int Tmax, int nh, int hd,
                                                                  float sgn, int zero_q) {
  const int dm = nh * hd;
  const int cpr = 3 * dm / 8;  // 16-byte chunks per qkv row
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * n * cpr) return;
  const int64_t row = i / cpr;  // b * n + r
  const int c = (int)(i - row * cpr);
  const int b = (int)(row / n), r = (int)(row - (int64_t)b * n);
  const int col = c * 8;
  const int l0 = lens0[b];
  const int cb = ext_clamp(n_new != nullptr ? n_new[b] : n, 0, n);
  const int lim = Tmax < rope_T ? Tmax : rope_T;
  const bool refused = l0 < 0 || (int64_t)l0 + cb > lim;  // nothing of this sequence is stored
  if (refused && r == 0 && c == 0) status[0] = 1;
  if (refused || r >= cb) {  // no cache row
    if (zero_q && col < dm) st_bf16x8(q_out + row * dm + col, zero_bf16x8());
    return;
  }
  const int t = l0 + r;
  bf16x8_t v = ld_bf16x8(qkv + row * ld_qkv + col);
  if (col < 2 * dm) {  // q | k: the rotation of rope_qk_kernel (attn.hip), same table loads, same rope8
    const int pair0 = (col % hd) / 2;
    const f32x4_t cs = *reinterpret_cast<const f32x4_t*>(rcos + (int64_t)t * (hd / 2) + pair0);
    const f32x4_t sn = *reinterpret_cast<const f32x4_t*>(rsin + (int64_t)t * (hd / 2) + pair0);
    v = rope8(v, cs, sn, sgn);
  }
  if (col < dm)
    st_bf16x8(q_out + row * dm + col, v);
  else
    st_bf16x8(kv + ((int64_t)b * Tmax + t) * ld_kv + (col - dm), v);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the FP8 cache: kv8[B, Tmax, ld_kv8] bytes, row = k codes dm | v codes dm | k scales dm/16 | v scales dm/16,
// e4m3fn codes under one E8M0 scale per 16 elements of a head (plm_fp8.h), quantised from the bf16 values the bf16 cache would hold
// ---------------------------------------------------------------------------------------------------------------------------------
// 16 bf16 values (two 16-byte chunks) -> 16 code bytes at dst and the block's scale byte at *sc: plain vector stores
__device__ __forceinline__ void kv8_store_block(bf16x8_t v0, bf16x8_t v1, uint8_t* dst, uint8_t* sc) {
  float f[16];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    f[e] = bf2f(v0[e]);
    f[8 + e] = bf2f(v1[e]);
  }
  u32x4_t q;
  const unsigned sb = kv8_block(f, q);
  *reinterpret_cast<u32x4_t*>(dst) = q;
  *sc = (uint8_t)sb;
}

// plm_kv8_append_rope_rows: kv_append_rope_rows_kernel with one thread per 16 columns (two of its chunks, one block of the cache);
// the same refusals, the same table loads and rope8 calls, so q_out and the values that are quantised are its bits
__global__ __launch_bounds__(256) void kv8_append_rope_rows_kernel(const uint16_t* __restrict__ qkv, int64_t ld_qkv,
                                                                   const int32_t* __restrict__ lens0, const int32_t* __restrict__ n_new,
                                                                   const float* __restrict__ rcos, const float* __restrict__ rsin, int rope_T,
                                                                   uint16_t* __restrict__ q_out, uint8_t* __restrict__ kv8, int64_t ld_kv8,
                                                                   int32_t* __restrict__ status, int B, int n, int Tmax, int nh, int hd,
                                                                   float sgn) {
  const int dm = nh * hd;
  const int upr = 3 * dm / 16;  // 16-column units per qkv row
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * n * upr) return;
  const int64_t row = i / upr;  // b * n + r
  const int c = (int)(i - row * upr);
  const int b = (int)(row / n), r = (int)(row - (int64_t)b * n);
  const int col = c * 16;
  const int l0 = lens0[b];
  const int cb = ext_clamp(n_new != nullptr ? n_new[b] : n, 0, n);
  const int lim = Tmax < rope_T ? Tmax : rope_T;
  const bool refused = l0 < 0 || (int64_t)l0 + cb > lim;  // nothing of this sequence is stored
  if (refused && r == 0 && c == 0) status[0] = 1;
  if (refused || r >= cb) {  // no cache row: a q row of zeros
    if (col < dm) {
      st_bf16x8(q_out + row * dm + col, zero_bf16x8());
      st_bf16x8(q_out + row * dm + col + 8, zero_bf16x8());
    }
    return;
  }
  const int t = l0 + r;
  bf16x8_t v0 = ld_bf16x8(qkv + row * ld_qkv + col), v1 = ld_bf16x8(qkv + row * ld_qkv + col + 8);
  if (col < 2 * dm) {
    const float* cp = rcos + (int64_t)t * (hd / 2) + (col % hd) / 2;
    const float* sp = rsin + (int64_t)t * (hd / 2) + (col % hd) / 2;
    v0 = rope8(v0, *reinterpret_cast<const f32x4_t*>(cp), *reinterpret_cast<const f32x4_t*>(sp), sgn);
    v1 = rope8(v1, *reinterpret_cast<const f32x4_t*>(cp + 4), *reinterpret_cast<const f32x4_t*>(sp + 4), sgn);
  }
  if (col < dm) {
    st_bf16x8(q_out + row * dm + col, v0);
    st_bf16x8(q_out + row * dm + col + 8, v1);
  } else {
    uint8_t* rowp = kv8 + ((int64_t)b * Tmax + t) * ld_kv8;
    kv8_store_block(v0, v1, rowp + (col - dm), rowp + 2 * dm + (col - dm) / 16);
  }
}

// plm_kv8_quant_rows / plm_kv8_dequant_rows: one thread per block of 16 of rows 0 .. T-1 of every sequence
__global__ __launch_bounds__(256) void kv8_quant_rows_kernel(const uint16_t* __restrict__ src, int64_t ld_src, uint8_t* __restrict__ kv8,
                                                             int64_t ld_kv8, int B, int T, int Tmax, int dm) {
  const int upr = 2 * dm / 16;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T * upr) return;
  const int64_t row = i / upr;  // b * T + t
  const int c = (int)(i - row * upr);
  const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
  const uint16_t* s = src + row * ld_src + c * 16;
  uint8_t* rowp = kv8 + ((int64_t)b * Tmax + t) * ld_kv8;
  kv8_store_block(ld_bf16x8(s), ld_bf16x8(s + 8), rowp + c * 16, rowp + 2 * dm + c);
}

__global__ __launch_bounds__(256) void kv8_dequant_rows_kernel(const uint8_t* __restrict__ kv8, int64_t ld_kv8, uint16_t* __restrict__ dst,
                                                               int64_t ld_dst, int B, int T, int Tmax, int dm) {
  const int upr = 2 * dm / 16;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T * upr) return;
  const int64_t row = i / upr;
  const int c = (int)(i - row * upr);
  const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
  const uint8_t* rowp = kv8 + ((int64_t)b * Tmax + t) * ld_kv8;
  const u32x4_t q = *reinterpret_cast<const u32x4_t*>(rowp + c * 16);
  const unsigned sb = rowp[2 * dm + c];
  uint16_t* d = dst + row * ld_dst + c * 16;
  st_bf16x8(d, kv8_deq8_bf16(u32x2_t{q[0], q[1]}, sb));
  st_bf16x8(d + 8, kv8_deq8_bf16(u32x2_t{q[2], q[3]}, sb));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_attn_decode
// ---------------------------------------------------------------------------------------------------------------------------------
// What a lane holds of one key row, by cache format: 8 elements of k and of v.  bf16: two 16-byte loads.  FP8: two 8-byte code loads
// and the two scale bytes of the blocks they lie in, dequantised on use - code * 2^(s - 127) is exact in fp32, so the kernel computes,
// bit for bit, what the bf16 instantiation computes on the dequantised cache.
template <typename KV>
struct DecRows;  // the DEC_UNROLL key rows a lane has in flight
template <>
struct DecRows<uint16_t> {
  bf16x8_t kk[DEC_UNROLL], vv[DEC_UNROLL];
  __device__ __forceinline__ void zero(int u) {
    kk[u] = zero_bf16x8();
    vv[u] = zero_bf16x8();
  }
  __device__ __forceinline__ void load(int u, const uint16_t* p, const uint16_t*, int dm) {
    kk[u] = ld_bf16x8(p);
    vv[u] = ld_bf16x8(p + dm);
  }
  __device__ __forceinline__ void prep(int) {}
  __device__ __forceinline__ float kx(int u, int e) const { return bf2f(kk[u][e]); }
  __device__ __forceinline__ float vx(int u, int e) const { return bf2f(vv[u][e]); }
};
template <>
struct DecRows<uint8_t> {
  u32x2_t kk[DEC_UNROLL], vv[DEC_UNROLL];
  unsigned ks[DEC_UNROLL], vs[DEC_UNROLL];
  float kf[8], vf[8];  // the row prep() dequantised last
  __device__ __forceinline__ void zero(int u) {
    kk[u] = u32x2_t{0u, 0u};
    vv[u] = u32x2_t{0u, 0u};
    ks[u] = vs[u] = 0u;
  }
  __device__ __forceinline__ void load(int u, const uint8_t* p, const uint8_t* sp, int dm) {  // sp: the k scale byte; + dm/16: the v scale byte
    kk[u] = *reinterpret_cast<const u32x2_t*>(p);
    vv[u] = *reinterpret_cast<const u32x2_t*>(p + dm);
    ks[u] = sp[0];
    vs[u] = sp[dm >> 4];
  }
  __device__ __forceinline__ void prep(int u) {
    kv8_deq8(kk[u], ks[u], kf);
    kv8_deq8(vv[u], vs[u], vf);
  }
  __device__ __forceinline__ float kx(int, int e) const { return kf[e]; }
  __device__ __forceinline__ float vx(int, int e) const { return vf[e]; }
};

// exp2(x - m) with the one hazard of an online softmax taken out: when nothing has been seen yet m is -inf and x may be too
// (-inf - -inf = NaN); subtracting 0 instead gives exp2(-inf) = 0, which is the right weight of an empty partial
__device__ __forceinline__ float dec_base(float m) { return m == -INFINITY ? 0.f : m; }

// Workspace: ml fp32 [B*nh, S, 2] (running maximum in log2 units, sum of 2^(s - m)) then acc fp32 [B*nh, S, hd] (sum of 2^(s - m) v).
// KV = uint16_t: the bf16 cache, ld_kv in elements; uint8_t: the FP8 cache, ld_kv in bytes.  One body: the key -> (wave, lane group)
// assignment, the loop and the order of every fp32 operation do not depend on the format.
template <int HD, typename KV>
__global__ __launch_bounds__(DEC_THREADS) void attn_decode_split_kernel(const uint16_t* __restrict__ q, const KV* __restrict__ kv,
                                                                        int64_t ld_kv, const int32_t* __restrict__ lens,
                                                                        float* __restrict__ ws_ml, float* __restrict__ ws_acc, int Tmax, int nh,
                                                                        int S, float c2) {
  constexpr int G = HD / 8;          // lanes per key row
  constexpr int KPW = PLM_WAVE / G;  // key rows per wave and load instruction
  __shared__ float s_ml[DEC_WAVES][2];
  __shared__ float s_acc[DEC_WAVES][HD];

  const int bh = blockIdx.x, s = blockIdx.y;
  const int b = bh / nh, h = bh - b * nh;
  const int tid = threadIdx.x, wave = tid / PLM_WAVE, lane = tid % PLM_WAVE;
  const int grp = lane / G, sub = lane % G;
  const int dm = nh * HD;

  int len = lens[b];
  len = len < 0 ? 0 : (len > Tmax ? Tmax : len);
  const int chunk = (len + S - 1) / S;
  const int k0 = min(s * chunk, len), k1 = min(k0 + chunk, len);  // this split's keys; empty when len < S * chunk

  // q slice of this lane, pre-scaled to log2 units
  float qf[8];
  {
    const bf16x8_t qv = ld_bf16x8(q + (int64_t)b * dm + h * HD + sub * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[e] = bf2f(qv[e]) * c2;
  }
  const KV* kbase = kv + (int64_t)b * Tmax * ld_kv + h * HD + sub * 8;  // + j * ld_kv: k of key j; + dm: its v
  // FP8: the scale byte of this lane's k block (+ j * ld_kv; + dm / 16: of its v block); the bf16 rows have none
  const KV* sbase = sizeof(KV) == 1 ? kv + (int64_t)b * Tmax * ld_kv + 2 * dm + ((h * HD + sub * 8) >> 4) : kbase;

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;

  for (int j0 = k0 + wave * (KPW * DEC_UNROLL); j0 < k1; j0 += DEC_WAVES * KPW * DEC_UNROLL) {
    DecRows<KV> rows;
    bool ok[DEC_UNROLL];
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {  // all loads first: the kernel lives on memory-level parallelism
      const int j = j0 + u * KPW + grp;
      ok[u] = j < k1;
      rows.zero(u);
      // rows at and beyond lens[b] are never read (they may hold anything, and j may be past Tmax)
      if (ok[u]) rows.load(u, kbase + (int64_t)j * ld_kv, sbase + (int64_t)j * ld_kv, dm);
    }
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      rows.prep(u);
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d = fmaf(qf[e], rows.kx(u, e), d);
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, PLM_WAVE);  // inside the lane group
      const float sc = ok[u] ? d : -INFINITY;
      const float mn = fmaxf(m, sc);
      const float base = dec_base(mn);
      const float alpha = __builtin_amdgcn_exp2f(m - base);
      const float p = __builtin_amdgcn_exp2f(sc - base);
      l = l * alpha + p;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = acc[e] * alpha + p * rows.vx(u, e);
      m = mn;
    }
  }

  // lane groups of a wave -> one partial (butterfly over the group index: every group ends with the same value)
#pragma unroll
  for (int o = G; o < PLM_WAVE; o <<= 1) {
    const float m2 = __shfl_xor(m, o, PLM_WAVE), l2 = __shfl_xor(l, o, PLM_WAVE);
    const float mn = fmaxf(m, m2), base = dec_base(mn);
    const float a = __builtin_amdgcn_exp2f(m - base), a2 = __builtin_amdgcn_exp2f(m2 - base);
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
  // waves -> the split's partial, in wave order
  if (tid < HD) {
    float mm = s_ml[0][0];
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) mm = fmaxf(mm, s_ml[w][0]);
    const float base = dec_base(mm);
    float ll = 0.f, a = 0.f;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) {
      const float sc = __builtin_amdgcn_exp2f(s_ml[w][0] - base);
      ll += s_ml[w][1] * sc;
      a += s_acc[w][tid] * sc;
    }
    const int64_t part = (int64_t)bh * S + s;
    if (tid == 0) {
      ws_ml[part * 2] = mm;
      ws_ml[part * 2 + 1] = ll;
    }
    ws_acc[part * HD + tid] = a;  // an empty split: (m = -inf, l = 0, acc = 0)
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_attn_extend
// ---------------------------------------------------------------------------------------------------------------------------------
// Workspace: acc fp32 [B*nh, S, n, hd] (sum of 2^(s - m) v) then ml fp32 [B*nh, S, n, 2] (running maximum in log2 units, sum of
// 2^(s - m)); rows r >= c_b are neither written nor read.
// KV as in attn_decode_split_kernel: the FP8 instantiation differs in the tile loads alone, which dequantise into the same LDS image.
template <int HD, typename KV>
__global__ __launch_bounds__(256, 2) void attn_extend_kernel(const uint16_t* __restrict__ q, const KV* __restrict__ kv, int64_t ld_kv,
                                                             const int32_t* __restrict__ lens0, const int32_t* __restrict__ n_new,
                                                             uint16_t* __restrict__ out, float* __restrict__ lse, float* __restrict__ ws_acc,
                                                             float* __restrict__ ws_ml, int n, int Tmax, int nh, int nqt, int S, float scale) {
  using TL = GenTile<HD>;
  __shared__ __attribute__((aligned(16))) char smem[2 * TL::BYTES];  // K | V
  constexpr int NKS = HD / 16, NDB = HD / 32;
  const int qt = (int)(blockIdx.x % nqt), bh = (int)(blockIdx.x / nqt), h = bh % nh, b = bh / nh, sp = blockIdx.y;
  const int dm = nh * HD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;

  const int l0 = ext_clamp(lens0[b], 0, Tmax);
  const int cb = ext_clamp(n_new != nullptr ? n_new[b] : n, 0, n);
  const int L = (int)min((int64_t)l0 + cb, (int64_t)Tmax);  // keys of the sequence; rows at and beyond L are never loaded
  const int chunk = (L + S - 1) / S;
  const int k0 = min(sp * chunk, L), k1 = min(k0 + chunk, L);  // this split's keys; empty when L < S * chunk

  const int q0 = qt * 128, r = q0 + wave * 32 + l31;
  const bool valid = r < cb;
  // the last key this lane's query may see inside the split (min(r, Tmax): no overflow for a huge n); -1: none
  const int lim = valid ? min(min(l0 + min(r, Tmax), Tmax - 1), k1 - 1) : -1;
  // the workgroup walks the split up to the last key its last valid row sees
  const int rlast = min(q0 + 127, cb - 1);
  const int kend = rlast < q0 ? k0 : min(k1, min(l0 + min(rlast, Tmax), Tmax - 1) + 1);

  const KV* kbase = kv + (int64_t)b * Tmax * ld_kv + h * HD;  // + j * ld_kv: k of key j; + dm: its v
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
  for (int kv0 = k0; kv0 < kend; kv0 += 64) {  // (bounds uniform over the workgroup)
    __syncthreads();                           // everyone is done with the previous tile
    if constexpr (sizeof(KV) == 2) {
      TL::load(sK, kbase, ld_kv, kv0, L - 1, tid);
      TL::load(sV, kbase + dm, ld_kv, kv0, L - 1, tid);
    } else {  // the scale bytes of this head: k's behind the 2 * dm code bytes of the row, v's dm / 16 further
      const KV* sbase = kv + (int64_t)b * Tmax * ld_kv + 2 * dm + ((h * HD) >> 4);
      TL::load(sK, kbase, sbase, ld_kv, kv0, L - 1, tid);
      TL::load(sV, kbase + dm, sbase + (dm >> 4), ld_kv, kv0, L - 1, tid);
    }
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
// the combine of both: one workgroup of HD threads per (sequence, head, query row), the S partials [B*nh, S, n] in split order
// ---------------------------------------------------------------------------------------------------------------------------------
// It takes the two halves of the workspace as two pointers, so decode keeps its ml | acc order and extend its acc | ml.
template <int HD>
__global__ __launch_bounds__(HD) void attn_cache_combine_kernel(const float* __restrict__ ws_acc, const float* __restrict__ ws_ml,
                                                                const int32_t* __restrict__ n_new, uint16_t* __restrict__ out,
                                                                float* __restrict__ lse, int n, int nh, int S) {
  const int r = (int)(blockIdx.x % n), bh = (int)(blockIdx.x / n), h = bh % nh, b = bh / nh, d = threadIdx.x;
  const int cb = ext_clamp(n_new != nullptr ? n_new[b] : n, 0, n);
  bf16_t o = f2bf(0.f);
  // a row at or beyond c_b (its partials, never written, are not read) and a row without any key (lens[b] == 0): the masked kernels'
  // rule for such a row, out = 0 and lse = +inf
  float Lq = INFINITY;
  if (r < cb) {
    float mm = -INFINITY;
    for (int s = 0; s < S; ++s) mm = fmaxf(mm, ws_ml[(((int64_t)bh * S + s) * n + r) * 2]);
    if (mm != -INFINITY) {
      float ll = 0.f, a = 0.f;
      for (int s = 0; s < S; ++s) {
        const int64_t part = ((int64_t)bh * S + s) * n + r;
        const float ms = ws_ml[part * 2];
        if (ms == -INFINITY) continue;  // an empty split carries no weight
        const float sc = __builtin_amdgcn_exp2f(ms - mm);
        ll += ws_ml[part * 2 + 1] * sc;
        a += ws_acc[part * HD + d] * sc;
      }
      o = f2bf(a / ll);
      Lq = mm + __builtin_amdgcn_logf(ll);  // base-2 LSE, plm_attn_fwd's convention
    }
  }
  reinterpret_cast<bf16_t*>(out)[((int64_t)b * n + r) * ((int64_t)nh * HD) + h * HD + d] = o;
  if (lse != nullptr && d == 0) lse[(int64_t)bh * n + r] = Lq;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side: the decode entry points are the chunk ones at n = 1
// ---------------------------------------------------------------------------------------------------------------------------------
// splits == 0: enough workgroups for two per CU, but no split shorter than 64 keys of the longest possible sequence.  A function of
// B, n, nh, Tmax and the CU count alone: what lens / n_new hold on the device is never consulted.
static int resolve_splits(int64_t B, int64_t n, int64_t nh, int64_t Tmax, int splits) {
  if (splits != 0) return splits;
  int64_t s = plm_cdiv(2 * CACHE_CUS, B * nh * plm_cdiv(n, 128));
  const int64_t cap = plm_cdiv(Tmax, 64);
  if (s > cap) s = cap;
  if (s > CACHE_MAX_SPLITS) s = CACHE_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

static bool shape_ok(int64_t B, int64_t n, int64_t nh, int64_t hd, int64_t Tmax) {
  const int64_t lim = (int64_t)1 << 31;
  return B > 0 && nh > 0 && Tmax > 0 && n > 0 && B < 65536 && nh < 65536 && Tmax < (1 << 24) && n < lim && B * n < lim && B * n * nh < lim &&
         (hd == 32 || hd == 64 || hd == 128);
}

static size_t ws_bytes(int64_t B, int64_t n, int64_t nh, int64_t hd, int S) {
  const size_t parts = (size_t)B * (size_t)nh * (size_t)S * (size_t)n;
  return (parts * (2 + (size_t)hd) * sizeof(float) + 15) / 16 * 16;
}

extern "C" size_t plm_attn_extend_workspace_bytes(int64_t B, int64_t n, int64_t nh, int64_t hd, int64_t Tmax, int splits) {
  if (!shape_ok(B, n, nh, hd, Tmax) || splits < 0 || splits > CACHE_MAX_SPLITS) return 0;
  return ws_bytes(B, n, nh, hd, resolve_splits(B, n, nh, Tmax, splits));
}

extern "C" size_t plm_attn_decode_workspace_bytes(int64_t B, int64_t nh, int64_t hd, int64_t Tmax, int splits) {
  return plm_attn_extend_workspace_bytes(B, 1, nh, hd, Tmax, splits);
}

// the append stage: every refusal, then the one launch.  `fn` is the entry point the caller sees.
static int append_rows(const char* fn, const uint16_t* qkv, int64_t ld_qkv, const int32_t* lens0, const int32_t* n_new, const float* rope_cos,
                       const float* rope_sin, int64_t rope_T, uint16_t* q_out, uint16_t* kv, int64_t ld_kv, int32_t* status, int64_t B, int64_t n,
                       int64_t Tmax, int64_t nh, int64_t hd, bool zero_q, void* stream) {
  PLM_REQUIRE(qkv && lens0 && rope_cos && rope_sin && q_out && kv && status, "%s: null pointer", fn);
  PLM_REQUIRE(hd == 32 || hd == 64 || hd == 128, "%s: head_dim %ld unsupported (32, 64, 128)", fn, (long)hd);
  PLM_REQUIRE(shape_ok(B, n, nh, hd, Tmax) && rope_T > 0 && rope_T < (1 << 24),
              "%s: bad shape B=%ld n=%ld Tmax=%ld nh=%ld rope_T=%ld (n >= 1, B*n < 2^31)", fn, (long)B, (long)n, (long)Tmax, (long)nh, (long)rope_T);
  PLM_REQUIRE(ld_qkv >= 3 * nh * hd && ld_qkv % 8 == 0 && ld_kv >= 2 * nh * hd && ld_kv % 8 == 0,
              "%s: row strides must be multiples of 8 and at least 3*nh*hd (qkv) / 2*nh*hd (kv)", fn);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(q_out) | reinterpret_cast<uintptr_t>(kv) |
                reinterpret_cast<uintptr_t>(rope_cos) | reinterpret_cast<uintptr_t>(rope_sin)) & 15) == 0,
              "%s: qkv, q_out, kv and the RoPE tables must be 16-byte aligned", fn);
  const int64_t blocks = plm_cdiv(B * n * (3 * nh * hd / 8), 256);
  PLM_REQUIRE(blocks < ((int64_t)1 << 31), "%s: bad shape: B*n*nh*hd too large for one launch", fn);
  hipLaunchKernelGGL(kv_append_rope_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, qkv, ld_qkv, lens0, n_new, rope_cos,
                     rope_sin, (int)rope_T, q_out, kv, ld_kv, status, (int)B, (int)n, (int)Tmax, (int)nh, (int)hd, 1.f, (int)zero_q);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" int plm_kv_append_rope(const uint16_t* qkv, int64_t ld_qkv, const int32_t* pos, const float* rope_cos, const float* rope_sin,
                                  int64_t rope_T, uint16_t* q_out, uint16_t* kv, int64_t ld_kv, int32_t* status, int64_t B, int64_t Tmax,
                                  int64_t nh, int64_t hd, void* stream) {
  return append_rows("plm_kv_append_rope", qkv, ld_qkv, pos, nullptr, rope_cos, rope_sin, rope_T, q_out, kv, ld_kv, status, B, 1, Tmax, nh, hd,
                     false, stream);
}

extern "C" int plm_kv_append_rope_rows(const uint16_t* qkv, int64_t ld_qkv, const int32_t* lens0, const int32_t* n_new, const float* rope_cos,
                                       const float* rope_sin, int64_t rope_T, uint16_t* q_out, uint16_t* kv, int64_t ld_kv, int32_t* status,
                                       int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd, void* stream) {
  return append_rows("plm_kv_append_rope_rows", qkv, ld_qkv, lens0, n_new, rope_cos, rope_sin, rope_T, q_out, kv, ld_kv, status, B, n, Tmax, nh,
                     hd, true, stream);
}


// the FP8 cache's stride rule: bytes, a multiple of 16 (the 16-byte code stores and 8-byte code loads stay aligned), at least the payload
static bool kv8_stride_ok(int64_t ld_kv8, int64_t dm) { return ld_kv8 % 16 == 0 && ld_kv8 >= kv8_row_payload(dm); }
#define KV8_STRIDE_MSG "%s: the FP8 cache's row stride must be a multiple of 16 bytes and at least 2*nh*hd + nh*hd/8"

extern "C" int plm_kv8_append_rope_rows(const uint16_t* qkv, int64_t ld_qkv, const int32_t* lens0, const int32_t* n_new, const float* rope_cos,
                                        const float* rope_sin, int64_t rope_T, uint16_t* q_out, uint8_t* kv8, int64_t ld_kv8, int32_t* status,
                                        int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd, void* stream) {
  const char* fn = "plm_kv8_append_rope_rows";
  PLM_REQUIRE(qkv && lens0 && rope_cos && rope_sin && q_out && kv8 && status, "%s: null pointer", fn);
  PLM_REQUIRE(hd == 32 || hd == 64 || hd == 128, "%s: head_dim %ld unsupported (32, 64, 128)", fn, (long)hd);
  PLM_REQUIRE(shape_ok(B, n, nh, hd, Tmax) && rope_T > 0 && rope_T < (1 << 24),
              "%s: bad shape B=%ld n=%ld Tmax=%ld nh=%ld rope_T=%ld (n >= 1, B*n < 2^31)", fn, (long)B, (long)n, (long)Tmax, (long)nh, (long)rope_T);
  PLM_REQUIRE(ld_qkv >= 3 * nh * hd && ld_qkv % 8 == 0, "%s: the qkv row stride must be a multiple of 8 and at least 3*nh*hd", fn);
  PLM_REQUIRE(kv8_stride_ok(ld_kv8, nh * hd), KV8_STRIDE_MSG, fn);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(q_out) | reinterpret_cast<uintptr_t>(kv8) |
                reinterpret_cast<uintptr_t>(rope_cos) | reinterpret_cast<uintptr_t>(rope_sin)) & 15) == 0,
              "%s: qkv, q_out, kv8 and the RoPE tables must be 16-byte aligned", fn);
  const int64_t blocks = plm_cdiv(B * n * (3 * nh * hd / 16), 256);
  PLM_REQUIRE(blocks < ((int64_t)1 << 31), "%s: bad shape: B*n*nh*hd too large for one launch", fn);
  hipLaunchKernelGGL(kv8_append_rope_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, qkv, ld_qkv, lens0, n_new, rope_cos,
                     rope_sin, (int)rope_T, q_out, kv8, ld_kv8, status, (int)B, (int)n, (int)Tmax, (int)nh, (int)hd, 1.f);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

// rows 0 .. T-1 of every sequence between bf16 k | v rows [B, T, ld] and the FP8 cache: the shared refusals
static int kv8_check_rows(const char* fn, const void* rows, int64_t ld, const void* kv8, int64_t ld_kv8, int64_t B, int64_t T, int64_t Tmax,
                          int64_t nh, int64_t hd) {
  PLM_REQUIRE(rows && kv8, "%s: null pointer", fn);
  PLM_REQUIRE(hd == 32 || hd == 64 || hd == 128, "%s: head_dim %ld unsupported (32, 64, 128)", fn, (long)hd);
  PLM_REQUIRE(shape_ok(B, T, nh, hd, Tmax) && T <= Tmax, "%s: bad shape B=%ld T=%ld Tmax=%ld nh=%ld (1 <= T <= Tmax, B*T < 2^31)", fn, (long)B,
              (long)T, (long)Tmax, (long)nh);
  PLM_REQUIRE(ld >= 2 * nh * hd && ld % 8 == 0, "%s: the bf16 row stride must be a multiple of 8 and at least 2*nh*hd", fn);
  PLM_REQUIRE(kv8_stride_ok(ld_kv8, nh * hd), KV8_STRIDE_MSG, fn);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(kv8)) & 15) == 0, "%s: the bf16 rows and kv8 must be 16-byte aligned",
              fn);
  PLM_REQUIRE(plm_cdiv(B * T * (nh * hd / 8), 256) < ((int64_t)1 << 31), "%s: bad shape: B*T*nh*hd too large for one launch", fn);
  return PLM_OK;
}

extern "C" int plm_kv8_quant_rows(const uint16_t* src, int64_t ld_src, uint8_t* kv8, int64_t ld_kv8, int64_t B, int64_t T, int64_t Tmax,
                                  int64_t nh, int64_t hd, void* stream) {
  if (const int e = kv8_check_rows("plm_kv8_quant_rows", src, ld_src, kv8, ld_kv8, B, T, Tmax, nh, hd)) return e;
  hipLaunchKernelGGL(kv8_quant_rows_kernel, dim3((unsigned)plm_cdiv(B * T * (nh * hd / 8), 256)), dim3(256), 0, (hipStream_t)stream, src, ld_src,
                     kv8, ld_kv8, (int)B, (int)T, (int)Tmax, (int)(nh * hd));
  PLM_CHECK_LAUNCH("plm_kv8_quant_rows");
  return PLM_OK;
}

extern "C" int plm_kv8_dequant_rows(const uint8_t* kv8, int64_t ld_kv8, uint16_t* dst, int64_t ld_dst, int64_t B, int64_t T, int64_t Tmax,
                                    int64_t nh, int64_t hd, void* stream) {
  if (const int e = kv8_check_rows("plm_kv8_dequant_rows", dst, ld_dst, kv8, ld_kv8, B, T, Tmax, nh, hd)) return e;
  hipLaunchKernelGGL(kv8_dequant_rows_kernel, dim3((unsigned)plm_cdiv(B * T * (nh * hd / 8), 256)), dim3(256), 0, (hipStream_t)stream, kv8, ld_kv8,
                     dst, ld_dst, (int)B, (int)T, (int)Tmax, (int)(nh * hd));
  PLM_CHECK_LAUNCH("plm_kv8_dequant_rows");
  return PLM_OK;
}

// the attention stage's refusals; *S is the resolved split count.  KV picks the cache format's stride rule.
template <typename KV>
static int check_attend(const char* fn, const uint16_t* q, const KV* kv, int64_t ld_kv, const int32_t* lens, const uint16_t* out, int64_t B,
                        int64_t n, int64_t Tmax, int64_t nh, int64_t hd, int splits, const void* workspace, size_t workspace_bytes, int* S) {
  PLM_REQUIRE(q && kv && lens && out && workspace, "%s: null pointer", fn);
  PLM_REQUIRE(hd == 32 || hd == 64 || hd == 128, "%s: head_dim %ld unsupported (32, 64, 128)", fn, (long)hd);
  PLM_REQUIRE(shape_ok(B, n, nh, hd, Tmax), "%s: bad shape B=%ld n=%ld Tmax=%ld nh=%ld (n >= 1, B*n < 2^31)", fn, (long)B, (long)n, (long)Tmax,
              (long)nh);
  if (sizeof(KV) == 2) PLM_REQUIRE(ld_kv >= 2 * nh * hd && ld_kv % 8 == 0, "%s: the cache's row stride must be a multiple of 8 and at least 2*nh*hd", fn);
  else PLM_REQUIRE(kv8_stride_ok(ld_kv, nh * hd), KV8_STRIDE_MSG, fn);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(kv) | reinterpret_cast<uintptr_t>(out) |
                reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
              "%s: q, kv, out and the workspace must be 16-byte aligned", fn);
  PLM_REQUIRE(splits >= 0 && splits <= CACHE_MAX_SPLITS, "%s: splits=%d out of range (0 = automatic, 1..%d forced)", fn, splits, CACHE_MAX_SPLITS);
  *S = resolve_splits(B, n, nh, Tmax, splits);
  const size_t need = ws_bytes(B, n, nh, hd, *S);
  if (workspace_bytes < need) {
    plm_set_error("%s: workspace of %zu bytes required, %zu given", fn, need, workspace_bytes);
    return PLM_E_WORKSPACE;
  }
  return PLM_OK;
}

template <int HD, typename KV>
static void dec_launch(const uint16_t* q, const KV* kv, int64_t ld_kv, const int32_t* lens, uint16_t* out, float* lse, int64_t B, int64_t Tmax,
                       int64_t nh, int S, float* ws, hipStream_t s) {
  float* ws_ml = ws;
  float* ws_acc = ws + (size_t)B * nh * S * 2;
  const float c2 = (1.f / sqrtf((float)HD)) * GLOG2E;
  hipLaunchKernelGGL((attn_decode_split_kernel<HD, KV>), dim3((unsigned)(B * nh), (unsigned)S), dim3(DEC_THREADS), 0, s, q, kv, ld_kv, lens, ws_ml,
                     ws_acc, (int)Tmax, (int)nh, S, c2);
  hipLaunchKernelGGL(attn_cache_combine_kernel<HD>, dim3((unsigned)(B * nh)), dim3(HD), 0, s, ws_acc, ws_ml, (const int32_t*)nullptr, out, lse, 1,
                     (int)nh, S);
}

// plm_attn_decode and plm_attn_decode_kv8: `fn` is the entry point the caller sees
template <typename KV>
static int attn_decode(const char* fn, const uint16_t* q, const KV* kv, int64_t ld_kv, const int32_t* lens, uint16_t* out, float* lse, int64_t B,
                       int64_t Tmax, int64_t nh, int64_t hd, int splits, void* workspace, size_t workspace_bytes, void* stream) {
  int S;
  if (const int e = check_attend(fn, q, kv, ld_kv, lens, out, B, 1, Tmax, nh, hd, splits, workspace, workspace_bytes, &S)) return e;
  hipStream_t s = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  if (hd == 32) dec_launch<32>(q, kv, ld_kv, lens, out, lse, B, Tmax, nh, S, ws, s);
  else if (hd == 64) dec_launch<64>(q, kv, ld_kv, lens, out, lse, B, Tmax, nh, S, ws, s);
  else dec_launch<128>(q, kv, ld_kv, lens, out, lse, B, Tmax, nh, S, ws, s);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" int plm_attn_decode(const uint16_t* q, const uint16_t* kv, int64_t ld_kv, const int32_t* lens, uint16_t* out, float* lse, int64_t B,
                               int64_t Tmax, int64_t nh, int64_t hd, int splits, void* workspace, size_t workspace_bytes, void* stream) {
  return attn_decode("plm_attn_decode", q, kv, ld_kv, lens, out, lse, B, Tmax, nh, hd, splits, workspace, workspace_bytes, stream);
}

extern "C" int plm_attn_decode_kv8(const uint16_t* q, const uint8_t* kv8, int64_t ld_kv8, const int32_t* lens, uint16_t* out, float* lse, int64_t B,
                                   int64_t Tmax, int64_t nh, int64_t hd, int splits, void* workspace, size_t workspace_bytes, void* stream) {
  return attn_decode("plm_attn_decode_kv8", q, kv8, ld_kv8, lens, out, lse, B, Tmax, nh, hd, splits, workspace, workspace_bytes, stream);
}

template <int HD, typename KV>
static void ext_launch(const uint16_t* q, const KV* kv, int64_t ld_kv, const int32_t* lens0, const int32_t* n_new, uint16_t* out, float* lse,
                       int64_t B, int64_t n, int64_t Tmax, int64_t nh, int S, float* ws, hipStream_t s) {
  float* ws_acc = ws;
  float* ws_ml = ws + (size_t)B * nh * S * n * HD;
  const int nqt = (int)plm_cdiv(n, 128);
  const float scale = 1.f / sqrtf((float)HD);
  hipLaunchKernelGGL((attn_extend_kernel<HD, KV>), dim3((unsigned)(B * nh * nqt), (unsigned)S), dim3(256), 0, s, q, kv, ld_kv, lens0, n_new, out,
                     lse, ws_acc, ws_ml, (int)n, (int)Tmax, (int)nh, nqt, S, scale);
  if (S > 1)
    hipLaunchKernelGGL(attn_cache_combine_kernel<HD>, dim3((unsigned)(B * nh * n)), dim3(HD), 0, s, ws_acc, ws_ml, n_new, out, lse, (int)n,
                       (int)nh, S);
}

template <typename KV>
static int attn_extend(const char* fn, const uint16_t* q, const KV* kv, int64_t ld_kv, const int32_t* lens0, const int32_t* n_new, uint16_t* out,
                       float* lse, int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd, int splits, void* workspace, size_t workspace_bytes,
                       void* stream) {
  int S;
  if (const int e = check_attend(fn, q, kv, ld_kv, lens0, out, B, n, Tmax, nh, hd, splits, workspace, workspace_bytes, &S)) return e;
  hipStream_t s = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  if (hd == 32) ext_launch<32>(q, kv, ld_kv, lens0, n_new, out, lse, B, n, Tmax, nh, S, ws, s);
  else if (hd == 64) ext_launch<64>(q, kv, ld_kv, lens0, n_new, out, lse, B, n, Tmax, nh, S, ws, s);
  else ext_launch<128>(q, kv, ld_kv, lens0, n_new, out, lse, B, n, Tmax, nh, S, ws, s);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" int plm_attn_extend(const uint16_t* q, const uint16_t* kv, int64_t ld_kv, const int32_t* lens0, const int32_t* n_new, uint16_t* out,
                               float* lse, int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd, int splits, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return attn_extend("plm_attn_extend", q, kv, ld_kv, lens0, n_new, out, lse, B, n, Tmax, nh, hd, splits, workspace, workspace_bytes, stream);
}

extern "C" int plm_attn_extend_kv8(const uint16_t* q, const uint8_t* kv8, int64_t ld_kv8, const int32_t* lens0, const int32_t* n_new,
                                   uint16_t* out, float* lse, int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd, int splits,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return attn_extend("plm_attn_extend_kv8", q, kv8, ld_kv8, lens0, n_new, out, lse, B, n, Tmax, nh, hd, splits, workspace, workspace_bytes, stream);
}
