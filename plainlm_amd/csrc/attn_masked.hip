// Attention under an ARBITRARY boolean mask (models/transformer.py:52-61 hands any bool [B,T,T] mask to SDPA): the dense, bit-packed mask mode.
// Head dims 32, 64 and 128; the same plain flash-style structure as attn_generic.hip (128-row query tiles of 4 waves x 32 rows, 64-key K / V
// tiles copied to LDS by the whole workgroup, S^T = K Q^T so a lane owns a query, V^T / Q^T / dO^T operands through ds_read_b64_tr_b16) and the
// same numerics contract (fp32 statistics, bf16 P / dS, base-2 LSE, deterministic: no atomics).
//
// The mask arrives packed by plm_attn_mask_pack (one launch): bits uint64 [M, T, ceil(T/64)] - bit j % 64 of word (m, i, j / 64) is
// mask[m, i, j], bits past T are 0 - and a tile class uint8 [M, ceil(T/128), ceil(T/64)] for the 128-query x 64-key tiles the kernels walk:
// 0 = no bit set (the tile is skipped by the whole workgroup before any load), 1 = every in-range bit set (the unmasked path: no word is read),
// 2 = mixed.  M = B (batch_stride 1) or 1 (batch_stride 0: one mask shared by every sequence).  Keys after the query are legal: every key tile
// up to T is walked.  A query row with no allowed key follows torch's SDPA: out = 0, LSE = +inf (so the backward's exp2(s c - lse) is exactly
// 0), and the row contributes nothing to dQ / dK / dV.  q and k arrive ROTATED; the backward kernels return the gradient w.r.t. the rotated q, k
// and plm_attn_bwd_masked applies the inverse rotation in place afterwards, as the generic family does.
#include "attn_gen_tile.h"

// the word of a class-1 tile: every key of the tile that exists
__device__ __forceinline__ uint64_t mask_full_word(int kv0, int T) {
  const int n = T - kv0;
  return n >= 64 ? ~0ull : ((1ull << n) - 1ull);
}

// ---------------------------------------------------------------------------------------------
// pack: bool [M, T, T] -> bits + tile class.  One workgroup per (m, 128-query tile, 64-key word column); wave w packs rows w*32 .. + 31 by one
// ballot per row (lane = key), lane r of the wave keeps row r's word and stores it.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn_mask_pack_kernel(const uint8_t* __restrict__ mask, uint64_t* __restrict__ bits,
                                                             uint8_t* __restrict__ tile_class, int T) {
  __shared__ int flags[4][2];
  const int W = (T + 63) / 64, NQT = (T + 127) / 128;
  const int jt = (int)(blockIdx.x % W), qt = (int)((blockIdx.x / W) % NQT);
  const int64_t m = blockIdx.x / ((unsigned)W * NQT);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = jt * 64 + lane, row0 = qt * 128 + wave * 32;
  const uint64_t full = mask_full_word(jt * 64, T);
  const uint8_t* src = mask + m * T * T;
  uint64_t mine = 0;
  bool any = false, all = true;
#pragma unroll 8
  for (int r = 0; r < 32; ++r) {
    const int row = row0 + r;
    const bool in = row < T;  // (wave-uniform)
    const uint64_t word = __ballot(in && col < T && src[(int64_t)min(row, T - 1) * T + min(col, T - 1)] != 0);
    if (lane == r) mine = word;
    any |= word != 0;
    all &= !in || word == full;
  }
  if (lane < 32 && row0 + lane < T) bits[(m * T + row0 + lane) * W + jt] = mine;
  if (lane == 0) {
    flags[wave][0] = any;
    flags[wave][1] = all;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool a = flags[0][0] | flags[1][0] | flags[2][0] | flags[3][0];
    const bool f = flags[0][1] & flags[1][1] & flags[2][1] & flags[3][1];
    tile_class[(m * NQT + qt) * W + jt] = a ? (f ? 1 : 2) : 0;
  }
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256, 2) void attn_fwd_masked_kernel(const uint16_t* __restrict__ qkv, const uint64_t* __restrict__ bits,
                                                                 const uint8_t* __restrict__ tile_class, int bstride, uint16_t* __restrict__ out,
                                                                 float* __restrict__ lse, int T, int nh, float scale) {
  using TL = GenTile<HD>;
  __shared__ __attribute__((aligned(16))) char smem[2 * TL::BYTES];  // K | V
  constexpr int NKS = HD / 16, NDB = HD / 32;
  const int ntile = (T + 127) / 128, W = (T + 63) / 64;
  const int tile = ntile - 1 - (int)(blockIdx.x / (gridDim.x / ntile));
  const int bh = blockIdx.x % (gridDim.x / ntile), h = bh % nh, b = bh / nh;
  const int dm = nh * HD, ld = 3 * dm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  const int q0 = tile * 128, qrow = q0 + wave * 32 + l31;
  const bool qvalid = qrow < T;
  const uint16_t* base = qkv + (int64_t)b * T * ld + h * HD;
  const int64_t mb = (int64_t)b * bstride;
  const uint64_t* wrow = bits + (mb * T + min(qrow, T - 1)) * W;
  const uint8_t* crow = tile_class + (mb * ntile + tile) * W;
  const float c2 = scale * GLOG2E;
  bf16x8_t qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) qf[ks] = qvalid ? ld_bf16x8(base + (int64_t)qrow * ld + ks * 16 + hi * 8) : zero_bf16x8();
  f32x16_t o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) gzero16(o[db]);
  float m = -INFINITY, lsum = 0.f;
  char* sK = smem;
  char* sV = smem + TL::BYTES;
  for (int jt = 0; jt < W; ++jt) {
    const int cls = crow[jt];  // (uniform over the workgroup)
    if (cls == 0) continue;    // no query of the tile sees a key of it: no load, no barrier
    const int kv0 = jt * 64;
    __syncthreads();  // everyone is done with the previous tile
    TL::load(sK, base + dm, ld, kv0, T - 1, tid);
    TL::load(sV, base + 2 * dm, ld, kv0, T - 1, tid);
    __syncthreads();
    const uint64_t word = !qvalid ? 0ull : cls == 1 ? mask_full_word(kv0, T) : wrow[jt];
    if (__ballot(word != 0) == 0) continue;  // none of this wave's 32 queries sees the tile (wave-uniform)
    f32x16_t s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      gzero16(s[kb]);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) s[kb] = mfma32(TL::rows(sK, kb * 32 + l31, ks, hi), qf[ks], s[kb]);
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const uint32_t w32 = (uint32_t)(word >> (kb * 32 + 4 * hi));  // key kv0 + kb*32 + mfma32_row(r, hi) is bit (r & 3) + 8 (r >> 2) of it
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (!((w32 >> ((r & 3) + 8 * (r >> 2))) & 1u)) s[kb][r] = -INFINITY;
        tmax = fmaxf(tmax, s[kb][r]);
      }
    }
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
      for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kb][r], c2, -m_safe));
        psum += p;
        pf[kb * 2 + (r >> 3)][r & 7] = f2bf(p);
      }
    lsum = lsum * alpha + psum;
    m = m_new;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
#pragma unroll
      for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
#pragma unroll
      for (int sp = 0; sp < 4; ++sp) o[db] = mfma32(TL::cols(sV, db, (sp >> 1) * 32 + (sp & 1) * 16 + 4 * hi, lane), pf[sp], o[db]);
    }
  }
  float l_lo, l_hi;
  half_pair(lsum, l_lo, l_hi);
  const float ltot = l_lo + l_hi;
  const bool empty = !(ltot > 0.f);  // no allowed key: out 0, LSE +inf (a row that sees a key sums at least the 1 of its maximum)
  const float inv = empty ? 0.f : 1.f / ltot;
  if (qvalid) {
    if (hi == 0) lse[((int64_t)b * nh + h) * T + qrow] = empty ? INFINITY : m + __builtin_amdgcn_logf(ltot);  // base-2 LSE
    uint16_t* orow = out + ((int64_t)b * T + qrow) * dm + h * HD;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = f2bf(o[db][4 * g + e] * inv);
        st_bf16x4(orow + db * 32 + 8 * g + 4 * hi, v);
      }
  }
}

// ---------------------------------------------------------------------------------------------
// backward dQ (w.r.t. the ROTATED q); publishes delta[q] = sum_d dO O (plain sign, every head dim)
// ---------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_masked_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ out,
                                                                    const uint16_t* __restrict__ dout, const float* __restrict__ lse,
                                                                    float* __restrict__ delta, const uint64_t* __restrict__ bits,
                                                                    const uint8_t* __restrict__ tile_class, int bstride,
                                                                    uint16_t* __restrict__ dqkv, int T, int nh, float scale) {
  using TL = GenTile<HD>;
  __shared__ __attribute__((aligned(16))) char smem[2 * TL::BYTES];
  constexpr int NKS = HD / 16, NDB = HD / 32;
  const int ntile = (T + 127) / 128, W = (T + 63) / 64;
  const int tile = ntile - 1 - (int)(blockIdx.x / (gridDim.x / ntile));
  const int bh = blockIdx.x % (gridDim.x / ntile), h = bh % nh, b = bh / nh;
  const int dm = nh * HD, ld = 3 * dm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  const int q0 = tile * 128, qrow = q0 + wave * 32 + l31;
  const bool qvalid = qrow < T;
  const uint16_t* base = qkv + (int64_t)b * T * ld + h * HD;
  const int64_t mb = (int64_t)b * bstride;
  const uint64_t* wrow = bits + (mb * T + min(qrow, T - 1)) * W;
  const uint8_t* crow = tile_class + (mb * ntile + tile) * W;
  const float c2 = scale * GLOG2E;
  bf16x8_t qf[NKS], dof[NKS];
  float part = 0.f;
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int d0 = ks * 16 + hi * 8;
    qf[ks] = qvalid ? ld_bf16x8(base + (int64_t)qrow * ld + d0) : zero_bf16x8();
    dof[ks] = qvalid ? ld_bf16x8(dout + ((int64_t)b * T + qrow) * dm + h * HD + d0) : zero_bf16x8();
    if (qvalid) {
      const bf16x8_t o8 = ld_bf16x8(out + ((int64_t)b * T + qrow) * dm + h * HD + d0);
#pragma unroll
      for (int e = 0; e < 8; ++e) part += bf2f(o8[e]) * bf2f(dof[ks][e]);
    }
  }
  float d_lo, d_hi;
  half_pair(part, d_lo, d_hi);
  const float Dq = d_lo + d_hi;
  const float Lq = qvalid ? lse[((int64_t)b * nh + h) * T + qrow] : INFINITY;  // +inf (empty row): every p below is exactly 0
  if (qvalid && hi == 0) delta[((int64_t)b * nh + h) * T + qrow] = Dq;
  f32x16_t dq[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) gzero16(dq[db]);
  char* sK = smem;
  char* sV = smem + TL::BYTES;
  for (int jt = 0; jt < W; ++jt) {
    const int cls = crow[jt];
    if (cls == 0) continue;
    const int kv0 = jt * 64;
    __syncthreads();
    TL::load(sK, base + dm, ld, kv0, T - 1, tid);
    TL::load(sV, base + 2 * dm, ld, kv0, T - 1, tid);
    __syncthreads();
    const uint64_t word = !qvalid ? 0ull : cls == 1 ? mask_full_word(kv0, T) : wrow[jt];
    if (__ballot(word != 0) == 0) continue;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      f32x16_t s, dp;
      gzero16(s);
      gzero16(dp);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        s = mfma32(TL::rows(sK, kb * 32 + l31, ks, hi), qf[ks], s);      // S^T[kv][q]
        dp = mfma32(TL::rows(sV, kb * 32 + l31, ks, hi), dof[ks], dp);   // dP^T[kv][q]
      }
      const uint32_t w32 = (uint32_t)(word >> (kb * 32 + 4 * hi));
      bf16x8_t dsf[2];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c2, -Lq));
        p = ((w32 >> ((r & 3) + 8 * (r >> 2))) & 1u) ? p : 0.f;
        dsf[r >> 3][r & 7] = f2bf(p * (dp[r] - Dq));
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int db = 0; db < NDB; ++db) dq[db] = mfma32(TL::cols(sK, db, kb * 32 + s2 * 16 + 4 * hi, lane), dsf[s2], dq[db]);  // dQ^T[d][q]
    }
  }
  if (qvalid) {
    uint16_t* orow = dqkv + ((int64_t)b * T + qrow) * ld + h * HD;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = f2bf(dq[db][4 * g + e] * scale);
        st_bf16x4(orow + db * 32 + 8 * g + 4 * hi, v);
      }
  }
}

// ---------------------------------------------------------------------------------------------
// backward dK / dV (dK w.r.t. the ROTATED k): one workgroup per 128 keys (4 waves x 32 keys in registers = key words 2 kt and 2 kt + 1), loops
// over EVERY 64-query tile; the tile's 64 x 2 mask words are staged in LDS next to its lse / delta (wave w reads the 32-bit half w of a row's
// pair: its own 32 keys)
// ---------------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256, 1) void attn_bwd_dkdv_masked_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout,
                                                                      const float* __restrict__ lse, const float* __restrict__ delta,
                                                                      const uint64_t* __restrict__ bits, const uint8_t* __restrict__ tile_class,
                                                                      int bstride, uint16_t* __restrict__ dqkv, int T, int nh, float scale) {
  using TL = GenTile<HD>;
  __shared__ __attribute__((aligned(16))) char smem[2 * TL::BYTES + 2 * 64 * 4 + 64 * 16];  // Q | dO | lse[64] | delta[64] | words[64][2]
  constexpr int NKS = HD / 16, NDB = HD / 32;
  const int ntile = (T + 127) / 128, W = (T + 63) / 64;
  const int kt = (int)(blockIdx.x / (gridDim.x / ntile));
  const int bh = blockIdx.x % (gridDim.x / ntile), h = bh % nh, b = bh / nh;
  const int dm = nh * HD, ld = 3 * dm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  const int kv0 = kt * 128, kvrow = kv0 + wave * 32 + l31;
  const bool kvalid = kvrow < T;
  const uint16_t* base = qkv + (int64_t)b * T * ld + h * HD;
  const uint16_t* dobase = dout + (int64_t)b * T * dm + h * HD;
  const int64_t mb = (int64_t)b * bstride;
  const uint64_t* wbase = bits + mb * T * W;
  const uint8_t* cbase = tile_class + mb * ntile * W;
  const int j0 = 2 * kt, j1 = 2 * kt + 1;  // key words of the workgroup (j1 == W when the last key tile holds 64 keys or fewer)
  const float c2 = scale * GLOG2E;
  bf16x8_t kf[NKS], vf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const uint16_t* p = base + (int64_t)kvrow * ld + ks * 16 + hi * 8;
    kf[ks] = kvalid ? ld_bf16x8(p + dm) : zero_bf16x8();
    vf[ks] = kvalid ? ld_bf16x8(p + 2 * dm) : zero_bf16x8();
  }
  f32x16_t dk[NDB], dv[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) {
    gzero16(dk[db]);
    gzero16(dv[db]);
  }
  char* sQ = smem;
  char* sDO = smem + TL::BYTES;
  float* sL = reinterpret_cast<float*>(smem + 2 * TL::BYTES);
  float* sD = sL + 64;
  uint64_t* sW = reinterpret_cast<uint64_t*>(sD + 64);
  const uint32_t* sW32 = reinterpret_cast<const uint32_t*>(sW);
  const int nqt = (T + 63) / 64;
  for (int jq = 0; jq < nqt; ++jq) {
    const int qt0 = jq * 64;
    const uint8_t* crow = cbase + (int64_t)(jq >> 1) * W;
    const int c0 = crow[j0], c1 = j1 < W ? crow[j1] : 0;  // (uniform over the workgroup)
    if (c0 == 0 && c1 == 0) continue;                     // no query of the 128-row tile sees any of these keys: no load, no barrier
    __syncthreads();
    TL::load(sQ, base, ld, qt0, T - 1, tid);
    TL::load(sDO, dobase, dm, qt0, T - 1, tid);
    if (tid < 64) {
      const int q = qt0 + tid, qc = min(q, T - 1);
      sL[tid] = lse[((int64_t)b * nh + h) * T + qc];
      sD[tid] = delta[((int64_t)b * nh + h) * T + qc];
      const uint64_t* wr = wbase + (int64_t)qc * W;
      uint64_t w0 = c0 == 0 ? 0ull : c0 == 1 ? mask_full_word(j0 * 64, T) : wr[j0];
      uint64_t w1 = c1 == 0 ? 0ull : c1 == 1 ? mask_full_word(j1 * 64, T) : wr[j1];
      if (q >= T) w0 = w1 = 0ull;
      sW[2 * tid] = w0;
      sW[2 * tid + 1] = w1;
    }
    __syncthreads();
    if ((wave >> 1 ? c1 : c0) == 0) continue;  // this wave's key word is invisible to the whole tile (wave-uniform)
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      f32x16_t s, dp;
      gzero16(s);
      gzero16(dp);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        s = mfma32(TL::rows(sQ, qb * 32 + l31, ks, hi), kf[ks], s);       // S[q][kv]
        dp = mfma32(TL::rows(sDO, qb * 32 + l31, ks, hi), vf[ks], dp);    // dP[q][kv]
      }
      bf16x8_t pf[2], dsf[2];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ql = qb * 32 + mfma32_row(r, hi);
        float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c2, -sL[ql]));
        p = ((sW32[4 * ql + wave] >> l31) & 1u) ? p : 0.f;
        pf[r >> 3][r & 7] = f2bf(p);
        dsf[r >> 3][r & 7] = f2bf(p * (dp[r] - sD[ql]));
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          dv[db] = mfma32(TL::cols(sDO, db, qb * 32 + s2 * 16 + 4 * hi, lane), pf[s2], dv[db]);   // dV^T[d][kv]
          dk[db] = mfma32(TL::cols(sQ, db, qb * 32 + s2 * 16 + 4 * hi, lane), dsf[s2], dk[db]);   // dK^T[d][kv]
        }
    }
  }
  if (kvalid) {
    uint16_t* krow = dqkv + ((int64_t)b * T + kvrow) * ld + dm + h * HD;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        bf16x4_t a, c;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] = f2bf(dk[db][4 * g + e] * scale);
          c[e] = f2bf(dv[db][4 * g + e]);
        }
        st_bf16x4(krow + db * 32 + 8 * g + 4 * hi, a);
        st_bf16x4(krow + dm + db * 32 + 8 * g + 4 * hi, c);
      }
  }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
void plm_rope_qk_inverse(uint16_t* qkv, const float* rope_cos, const float* rope_sin, int64_t B, int64_t T, int64_t nh, int64_t hd, hipStream_t s);

static inline bool mask_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline int64_t mask_words(int64_t T) { return (T + 63) / 64; }
static inline int64_t mask_bits_bytes(int64_t M, int64_t T) { return M * T * mask_words(T) * 8; }
static inline int64_t mask_class_bytes(int64_t M, int64_t T) { return M * ((T + 127) / 128) * mask_words(T); }

static int check_masked_shape(const char* name, int64_t B, int64_t T, int64_t nh, int64_t hd, int64_t batch_stride) {
  PLM_REQUIRE(hd == 32 || hd == 64 || hd == 128, "%s: head_dim %ld unsupported (32, 64, 128)", name, (long)hd);
  PLM_REQUIRE(B > 0 && T > 0 && nh > 0 && B < 65536 && nh < 65536 && T < (1 << 20), "%s: bad shape B=%ld T=%ld nh=%ld", name, (long)B, (long)T,
              (long)nh);
  PLM_REQUIRE(T % 4 == 0, "%s: T=%ld must be a multiple of 4", name, (long)T);
  PLM_REQUIRE(batch_stride == 0 || batch_stride == 1, "%s: batch_stride %ld must be 0 (one shared mask) or 1 (one mask per sequence)", name,
              (long)batch_stride);
  PLM_REQUIRE(B * nh * ((T + 127) / 128) < ((int64_t)1 << 31), "%s: grid too large", name);
  return PLM_OK;
}

extern "C" int64_t plm_attn_mask_bytes(int64_t B, int64_t T) {
  if (B <= 0 || T <= 0 || T % 4 != 0) return 0;
  return (mask_bits_bytes(B, T) + mask_class_bytes(B, T) + 15) & ~(int64_t)15;
}

extern "C" int plm_attn_mask_pack(const uint8_t* mask, int64_t batch_stride, uint64_t* bits, uint8_t* tile_class, int64_t B, int64_t T,
                                  void* stream) {
  PLM_REQUIRE(mask && bits && tile_class, "plm_attn_mask_pack: null pointer");
  PLM_REQUIRE(mask_aligned16(bits) && mask_aligned16(tile_class), "plm_attn_mask_pack: bits and tile_class must be 16-byte aligned");
  if (int rc = check_masked_shape("plm_attn_mask_pack", B, T, 1, 64, batch_stride)) return rc;
  const int64_t M = batch_stride ? B : 1;
  const int64_t grid = M * ((T + 127) / 128) * mask_words(T);
  PLM_REQUIRE(grid < ((int64_t)1 << 31), "plm_attn_mask_pack: B x T too large");
  hipLaunchKernelGGL(attn_mask_pack_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, mask, bits, tile_class, (int)T);
  PLM_CHECK_LAUNCH("plm_attn_mask_pack");
  return PLM_OK;
}

extern "C" int plm_attn_fwd_masked(const uint16_t* qkv, const uint64_t* bits, const uint8_t* tile_class, int64_t batch_stride, uint16_t* out,
                                   float* lse, int64_t B, int64_t T, int64_t nh, int64_t hd, void* stream) {
  PLM_REQUIRE(qkv && bits && tile_class && out && lse, "plm_attn_fwd_masked: null pointer");
  PLM_REQUIRE(mask_aligned16(qkv) && mask_aligned16(out) && mask_aligned16(bits) && mask_aligned16(tile_class),
              "plm_attn_fwd_masked: qkv, out, bits and tile_class must be 16-byte aligned");
  if (int rc = check_masked_shape("plm_attn_fwd_masked", B, T, nh, hd, batch_stride)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(plm_cdiv(T, 128) * nh * B)), block(256);
  const float scale = 1.f / sqrtf((float)hd);
  const int bs = (int)batch_stride, Ti = (int)T, nhi = (int)nh;
  if (hd == 32) hipLaunchKernelGGL(attn_fwd_masked_kernel<32>, grid, block, 0, s, qkv, bits, tile_class, bs, out, lse, Ti, nhi, scale);
  else if (hd == 64) hipLaunchKernelGGL(attn_fwd_masked_kernel<64>, grid, block, 0, s, qkv, bits, tile_class, bs, out, lse, Ti, nhi, scale);
  else hipLaunchKernelGGL(attn_fwd_masked_kernel<128>, grid, block, 0, s, qkv, bits, tile_class, bs, out, lse, Ti, nhi, scale);
  PLM_CHECK_LAUNCH("plm_attn_fwd_masked");
  return PLM_OK;
}

template <int HD>
static void bwd_masked_launch(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse, float* delta, const uint64_t* bits,
                              const uint8_t* tile_class, int bs, uint16_t* dqkv, int64_t B, int64_t T, int64_t nh, hipStream_t s) {
  const dim3 grid((unsigned)(plm_cdiv(T, 128) * nh * B)), block(256);
  const float scale = 1.f / sqrtf((float)HD);
  hipLaunchKernelGGL(attn_bwd_dq_masked_kernel<HD>, grid, block, 0, s, qkv, out, dout, lse, delta, bits, tile_class, bs, dqkv, (int)T, (int)nh, scale);
  hipLaunchKernelGGL(attn_bwd_dkdv_masked_kernel<HD>, grid, block, 0, s, qkv, dout, lse, delta, bits, tile_class, bs, dqkv, (int)T, (int)nh, scale);
}

extern "C" int plm_attn_bwd_masked(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse, const float* rope_cos,
                                   const float* rope_sin, const uint64_t* bits, const uint8_t* tile_class, int64_t batch_stride, uint16_t* dqkv,
                                   float* delta, int64_t B, int64_t T, int64_t nh, int64_t hd, void* stream) {
  PLM_REQUIRE(qkv && out && dout && lse && rope_cos && rope_sin && bits && tile_class && dqkv && delta, "plm_attn_bwd_masked: null pointer");
  PLM_REQUIRE(mask_aligned16(qkv) && mask_aligned16(out) && mask_aligned16(dout) && mask_aligned16(dqkv) && mask_aligned16(rope_cos) &&
                  mask_aligned16(rope_sin) && mask_aligned16(bits) && mask_aligned16(tile_class),
              "plm_attn_bwd_masked: qkv, out, dout, dqkv, the RoPE tables, bits and tile_class must be 16-byte aligned");
  if (int rc = check_masked_shape("plm_attn_bwd_masked", B, T, nh, hd, batch_stride)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int bs = (int)batch_stride;
  if (hd == 32) bwd_masked_launch<32>(qkv, out, dout, lse, delta, bits, tile_class, bs, dqkv, B, T, nh, s);
  else if (hd == 64) bwd_masked_launch<64>(qkv, out, dout, lse, delta, bits, tile_class, bs, dqkv, B, T, nh, s);
  else bwd_masked_launch<128>(qkv, out, dout, lse, delta, bits, tile_class, bs, dqkv, B, T, nh, s);
  // the kernels return the gradient w.r.t. the ROTATED q, k; the rotation is orthogonal, so its backward is the inverse rotation
  plm_rope_qk_inverse(dqkv, rope_cos, rope_sin, B, T, nh, hd, s);
  PLM_CHECK_LAUNCH("plm_attn_bwd_masked");
  return PLM_OK;
}
