// Beam-search decode attention for gfx950: the G beams of a prompt attend the prompt's k | v rows, held once in the
// prefix cache, followed by the rows of their HISTORY in the suffix caches of the prompt's G slots.  Beam search re-parents every beam at
// every step; instead of gathering suffix caches, an ancestor table anc uint8 [P*G, Ts_max] names, for beam g and generated token j, the
// slot whose row j holds that token.  Beams that share an ancestor share its rows, so the live rows of a prompt are a small trie.
// plm_attn_decode_beam is three launches: attn_shared.hip's prefix kernel, the suffix kernel below, attn_cache.hip's combine over the
// S_p + S_s partials of every (beam, head) - prefix partials first.
//
// attn_beam_suffix_kernel.  The grid is (P * nh) x S_s: a workgroup takes one prompt, one head and one range of 32-row tiles of the suffix.
// A key tile is 32 consecutive rows of ONE slot: contiguous in memory, loaded straight into the A operand of v_mfma_f32_32x32x16_bf16 as
// the prefix kernel loads K; the G <= 32 queries of the prompt are the B operand, so S^T = K Q^T gives every lane 16 scores of ITS beam
// (lane & 31).  The lane's mask for the tile is one word: bit r = (anc[g][j0 + r] == slot).  The 32 table bytes of a tile are read once
// per row tile and serve every slot.  A (slot, tile) pair that no beam attends - a wave-uniform ballot of the mask words - is skipped
// before any K or V byte is fetched: once the beams have collapsed onto a common ancestor, all but one slot of an old tile are dead.
// Masked scores are set to -inf BEFORE the running maximum, so a beam's numbers are a function of its own keys alone; a pair that is live
// for other beams is the identity on this one (alpha = 1, p = 0).
// Wave w takes the slots w, w + 4, .. of every tile of the range, in that fixed order, with a private online-softmax state (m, l, O) and
// a private V tile in LDS (the transposed read needs LDS; the wave that wrote a tile is the only reader, so a wavefront-scope fence
// orders it).  No barrier and no atomic in the loop.  After it the four states meet in LDS and are merged IN WAVE ORDER by the thread
// that owns the element; one fp32 partial (m, l, acc[hd]) per (beam, head, split) goes to the workspace in plm_attn_decode's layout.
// Safety rules (the extend and shared kernels'): row indices are clamped to the last valid row lens_s - 1, so a row at or beyond the
// length never reaches LDS or an MFMA operand; table bytes at or beyond the length are not read (they count as 0xFF, no slot); an entry
// >= G matches no slot; the m_safe guard; columns g >= G are zero queries, match nothing and write nothing.
// Built without packed fp32 VALU ops like attn_shared.hip (Makefile), for the same softmax arithmetic.
#include "attn_gen_tile.h"
#include "attn_cache.h"

#include "../../include/plainlm_hip.h"

#define BMA_THREADS 256
#define BMA_WAVES 4
#define BMA_Q 32     // beams per prompt at most: the N of the 32x32 MFMA
#define BMA_TILE 32  // rows of a key tile: the M of the 32x32 MFMA
#define BMA_PAD 4    // floats between the merge rows in LDS

__device__ __forceinline__ void bma_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int HD>
__global__ __launch_bounds__(BMA_THREADS) void attn_beam_suffix_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ kv, int64_t ld_kv,
                                                                       const int32_t* __restrict__ lens_s, const uint8_t* __restrict__ anc,
                                                                       float* __restrict__ ws_ml, float* __restrict__ ws_acc, int G, int Tmax, int nh,
                                                                       int S, int Stot, int part_off, float scale) {
  using TL = GenTile<HD>;
  constexpr int NKS = HD / 16, NDB = HD / 32, LDO = HD + BMA_PAD;
  constexpr int VT = BMA_TILE * TL::ROWB;  // bytes of a wave's V tile
  constexpr int MERGE = BMA_WAVES * BMA_Q * LDO * 4;
  constexpr int SMEM = BMA_WAVES * VT > MERGE ? BMA_WAVES * VT : MERGE;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];  // one V tile per wave; after the loop: O of every wave
  __shared__ float s_ml[BMA_WAVES][BMA_Q][2];

  const int h = (int)(blockIdx.x % nh), p = (int)(blockIdx.x / nh), sp = blockIdx.y;
  const int dm = nh * HD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;

  const int L = min(max(lens_s[(int64_t)p * G], 0), Tmax);  // suffix rows of the prompt (every slot holds as many); rows >= L are never loaded
  const int ntile = (L + BMA_TILE - 1) / BMA_TILE, tchunk = (ntile + S - 1) / S;
  const int t0 = min(sp * tchunk, ntile), t1 = min(t0 + tchunk, ntile);  // this split's row tiles

  const int g = l31;  // this lane's beam
  const bool valid = g < G;
  const int64_t seq0 = (int64_t)p * G;
  bf16x8_t qf[NKS];
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) qf[ks] = valid ? ld_bf16x8(q + (seq0 + g) * dm + h * HD + ks * 16 + hi * 8) : zero_bf16x8();
  const uint8_t* arow = anc + (seq0 + (valid ? g : 0)) * Tmax;

  const float c2 = scale * GLOG2E;
  f32x16_t o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) gzero16(o[db]);
  float m = -INFINITY, lsum = 0.f;
  char* sV = smem + wave * VT;

  for (int t = t0; t < t1; ++t) {  // (uniform over the workgroup; 0 <= j0 < L, so L >= 1 here)
    const int j0 = t * BMA_TILE;
    unsigned aw[8];  // the beam's slots of rows j0 .. j0 + 31, four to a word
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      unsigned x = 0u;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int j = j0 + 4 * w + b;
        const unsigned v = (valid && j < L) ? (unsigned)arow[j] : 0xFFu;
        x |= v << (8 * b);
      }
      aw[w] = x;
    }
    for (int s = wave; s < G; s += BMA_WAVES) {  // (uniform over the wave)
      unsigned word = 0u;  // bit r: this beam attends row j0 + r of slot s
#pragma unroll
      for (int r = 0; r < 32; ++r) word |= (unsigned)(((aw[r >> 2] >> (8 * (r & 3))) & 0xFFu) == (unsigned)s) << r;
      if (__ballot(word != 0u) == 0ull) continue;  // no beam attends the pair: nothing of it is fetched

      const uint16_t* kbase = kv + (seq0 + s) * Tmax * ld_kv + h * HD;  // + j * ld_kv: k of slot s's row j; + dm: its v
      bf16x8_t kf[NKS];
      {
        const uint16_t* kr = kbase + (int64_t)min(j0 + l31, L - 1) * ld_kv + hi * 8;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) kf[ks] = ld_bf16x8(kr + ks * 16);
      }
      bma_wave_sync();  // the reads of the previous tile were issued before these writes, and the LDS keeps a wave's order
      {
        constexpr int CPR = HD / 8;  // 16-byte chunks per row
#pragma unroll
        for (int it = 0; it < CPR / 2; ++it) {
          const int c = it * 64 + lane, r = c / CPR, k = c - r * CPR;
          *reinterpret_cast<bf16x8_t*>(sV + r * TL::ROWB + k * 16) = ld_bf16x8(kbase + dm + (int64_t)min(j0 + r, L - 1) * ld_kv + k * 8);
        }
      }
      bma_wave_sync();
      f32x16_t sc;
      gzero16(sc);
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) sc = mfma32(kf[ks], qf[ks], sc);
      float tmax = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if (((word >> mfma32_row(e, hi)) & 1u) == 0u) sc[e] = -INFINITY;  // another beam's row, or a row at or beyond L
        tmax = fmaxf(tmax, sc[e]);
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
      bf16x8_t pf[2];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float pe = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[e], c2, -m_safe));
        psum += pe;
        pf[e >> 3][e & 7] = f2bf(pe);
      }
      lsum = lsum * alpha + psum;
      m = m_new;
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
#pragma unroll
        for (int e = 0; e < 16; ++e) o[db][e] *= alpha;
#pragma unroll
        for (int u = 0; u < 2; ++u) o[db] = mfma32(TL::cols(sV, db, u * 16 + 4 * hi, lane), pf[u], o[db]);
      }
    }
  }
  float l_lo, l_hi;
  half_pair(lsum, l_lo, l_hi);
  const float ltot = l_lo + l_hi;

  // the four wave states -> LDS: O[wave][beam][head dim] over the V tiles, once every wave is done with its own
  __syncthreads();
  float* s_o = reinterpret_cast<float*>(smem);
  if (hi == 0) {
    s_ml[wave][l31][0] = m;
    s_ml[wave][l31][1] = ltot;
  }
  {
    float* orow = s_o + (wave * BMA_Q + l31) * LDO;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        f32x4_t v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = o[db][4 * gg + e];
        *reinterpret_cast<f32x4_t*>(orow + db * 32 + 8 * gg + 4 * hi) = v;
      }
  }
  __syncthreads();
  // merge in wave order: thread (beam j, slice c) owns HD / 8 head dims of beam j
  constexpr int SL = HD / 8;
  const int j = tid >> 3, c = (tid & 7) * SL;
  if (j >= G) return;  // a query column past the beams: no partial
  float mm = s_ml[0][j][0];
#pragma unroll
  for (int w = 1; w < BMA_WAVES; ++w) mm = fmaxf(mm, s_ml[w][j][0]);
  const float base = (mm == -INFINITY) ? 0.f : mm;
  float ll = 0.f, a[SL];
#pragma unroll
  for (int e = 0; e < SL; ++e) a[e] = 0.f;
#pragma unroll
  for (int w = 0; w < BMA_WAVES; ++w) {
    const float wsc = __builtin_amdgcn_exp2f(s_ml[w][j][0] - base);  // a wave without a live pair: m = -inf, weight 0
    ll += s_ml[w][j][1] * wsc;
    const float* orow = s_o + (w * BMA_Q + j) * LDO + c;
#pragma unroll
    for (int e = 0; e < SL; ++e) a[e] += orow[e] * wsc;
  }
  const int64_t part = ((seq0 + j) * nh + h) * Stot + part_off + sp;  // an empty split: (m = -inf, l = 0, acc = 0)
  if ((tid & 7) == 0) {
    ws_ml[part * 2] = mm;
    ws_ml[part * 2 + 1] = ll;
  }
#pragma unroll
  for (int e = 0; e < SL; ++e) ws_acc[part * HD + c + e] = a[e];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
// splits_s == 0: enough workgroups for two per CU, but no split shorter than two row tiles of the longest possible suffix.  A function of
// P, nh, Ts_max and the CU count alone.
static int beam_resolve_splits_s(int64_t P, int64_t nh, int64_t Ts_max, int splits_s) {
  if (splits_s != 0) return splits_s;
  int64_t s = plm_cdiv(2 * CACHE_CUS, P * nh);
  const int64_t cap = plm_cdiv(Ts_max, 2 * BMA_TILE);
  if (s > cap) s = cap;
  if (s > CACHE_MAX_SPLITS) s = CACHE_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

static bool beam_shape_ok(int64_t P, int64_t G, int64_t nh, int64_t hd, int64_t Tp_max, int64_t Ts_max, int splits_p, int splits_s) {
  return P > 0 && P < 65536 && G >= 1 && G <= BMA_Q && cache_shape_ok(P, 1, nh, hd, Tp_max) && cache_shape_ok(P * G, 1, nh, hd, Ts_max) &&
         P * nh < ((int64_t)1 << 31) && splits_p >= 0 && splits_p <= CACHE_MAX_SPLITS && splits_s >= 0 && splits_s <= CACHE_MAX_SPLITS;
}

extern "C" size_t plm_attn_decode_beam_workspace_bytes(int64_t P, int64_t G, int64_t nh, int64_t hd, int64_t Tp_max, int64_t Ts_max, int splits_p,
                                                       int splits_s) {
  if (!beam_shape_ok(P, G, nh, hd, Tp_max, Ts_max, splits_p, splits_s)) return 0;
  return cache_ws_bytes(P * G, 1, nh, hd, shared_resolve_splits_p(P, G, nh, Tp_max, splits_p) + beam_resolve_splits_s(P, nh, Ts_max, splits_s));
}

template <int HD>
static void bma_launch(const uint16_t* q, const uint16_t* kv_s, int64_t ld_kv_s, const int32_t* lens_s, const uint8_t* anc, float* ws_ml, float* ws_acc,
                       int64_t P, int64_t G, int64_t Ts_max, int64_t nh, int Ss, int Stot, int Sp, hipStream_t s) {
  hipLaunchKernelGGL(attn_beam_suffix_kernel<HD>, dim3((unsigned)(P * nh), (unsigned)Ss), dim3(BMA_THREADS), 0, s, q, kv_s, ld_kv_s, lens_s, anc, ws_ml,
                     ws_acc, (int)G, (int)Ts_max, (int)nh, Ss, Stot, Sp, 1.f / sqrtf((float)HD));
}

extern "C" int plm_attn_decode_beam(const uint16_t* q, const uint16_t* kv_p, int64_t ld_kv_p, const int32_t* lens_p, const uint16_t* kv_s,
                                    int64_t ld_kv_s, const int32_t* lens_s, const uint8_t* anc, uint16_t* out, float* lse, int64_t P, int64_t G,
                                    int64_t Tp_max, int64_t Ts_max, int64_t nh, int64_t hd, int splits_p, int splits_s, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  const char* fn = "plm_attn_decode_beam";
  PLM_REQUIRE(q && kv_p && lens_p && kv_s && lens_s && anc && out && workspace, "%s: null pointer", fn);
  PLM_REQUIRE(hd == 32 || hd == 64 || hd == 128, "%s: head_dim %ld unsupported (32, 64, 128)", fn, (long)hd);
  PLM_REQUIRE(G >= 1 && G <= BMA_Q, "%s: G=%ld beams per prompt unsupported (1 .. %d: one MFMA tile of queries)", fn, (long)G, BMA_Q);
  PLM_REQUIRE(splits_p >= 0 && splits_p <= CACHE_MAX_SPLITS && splits_s >= 0 && splits_s <= CACHE_MAX_SPLITS,
              "%s: splits_p=%d / splits_s=%d out of range (0 = automatic, 1..%d forced)", fn, splits_p, splits_s, CACHE_MAX_SPLITS);
  PLM_REQUIRE(beam_shape_ok(P, G, nh, hd, Tp_max, Ts_max, splits_p, splits_s), "%s: bad shape P=%ld G=%ld Tp_max=%ld Ts_max=%ld nh=%ld", fn, (long)P,
              (long)G, (long)Tp_max, (long)Ts_max, (long)nh);
  PLM_REQUIRE(ld_kv_p >= 2 * nh * hd && ld_kv_p % 8 == 0 && ld_kv_s >= 2 * nh * hd && ld_kv_s % 8 == 0,
              "%s: the caches' row strides must be multiples of 8 and at least 2*nh*hd", fn);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(kv_p) | reinterpret_cast<uintptr_t>(kv_s) | reinterpret_cast<uintptr_t>(out) |
                reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
              "%s: q, kv_p, kv_s, out and the workspace must be 16-byte aligned", fn);
  const int Sp = shared_resolve_splits_p(P, G, nh, Tp_max, splits_p), Ss = beam_resolve_splits_s(P, nh, Ts_max, splits_s);
  const int Stot = Sp + Ss;
  const size_t need = cache_ws_bytes(P * G, 1, nh, hd, Stot);
  if (workspace_bytes < need) {
    plm_set_error("%s: workspace of %zu bytes required, %zu given", fn, need, workspace_bytes);
    return PLM_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* ws_ml = static_cast<float*>(workspace);
  float* ws_acc = ws_ml + (size_t)P * G * nh * Stot * 2;
  shared_prefix_launch(q, kv_p, ld_kv_p, lens_p, ws_ml, ws_acc, P, G, Tp_max, nh, hd, Sp, Stot, s);
  if (hd == 32) bma_launch<32>(q, kv_s, ld_kv_s, lens_s, anc, ws_ml, ws_acc, P, G, Ts_max, nh, Ss, Stot, Sp, s);
  else if (hd == 64) bma_launch<64>(q, kv_s, ld_kv_s, lens_s, anc, ws_ml, ws_acc, P, G, Ts_max, nh, Ss, Stot, Sp, s);
  else bma_launch<128>(q, kv_s, ld_kv_s, lens_s, anc, ws_ml, ws_acc, P, G, Ts_max, nh, Ss, Stot, Sp, s);
  cache_combine_launch(ws_acc, ws_ml, out, lse, P * G, nh, hd, Stot, s);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}
