// KV-cached generation for gfx950: the append of one rotated token per sequence into the per-layer cache, and
// attention of one query row per sequence over that cache (flash-decoding: split the keys, combine the partial softmaxes).
//
// Cache: kv[B, Tmax, ld_kv] bf16, row (b, j) = the k | v column blocks (2 * nh * hd values) of token j of sequence b, k already rotated -
// the bits plm_qkv_rope_bf16 leaves in columns [nh*hd, 3*nh*hd) of its output.  Nothing is transposed.
//
// The decode kernel is a bandwidth problem (one q row against lens[b] rows of 2 * hd * 2 bytes per head), so there is no MFMA in it: a
// group of hd / 8 lanes owns one key row, every lane loads 16 bytes of k and 16 bytes of v, the dot product is 8 VALU FMAs plus a butterfly
// inside the group, and the softmax is an online base-2 softmax in fp32 (P is never rounded to bf16).  No atomics: every partial is written
// by one workgroup and the combine walks them in split order, so the result is bit-reproducible and, for a fixed split count, independent
// of what the other sequences hold.
#include "plm_device.h"

#include "../../include/plainlm_hip.h"

#define DEC_THREADS 256
#define DEC_WAVES (DEC_THREADS / PLM_WAVE)
#define DEC_UNROLL 4
#define DEC_MAX_SPLITS 64
// the automatic split rule knows the device by this one number (MI355X: 256 CUs); nothing is queried, nothing is read back
#define DEC_CUS 256
static constexpr float DEC_LOG2E = 1.4426950408889634f;

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_kv_append_rope: one thread per 16-byte chunk of a qkv row
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kv_append_rope_kernel(const uint16_t* __restrict__ qkv, int64_t ld_qkv, const int32_t* __restrict__ pos,
                                                             const float* __restrict__ rcos, const float* __restrict__ rsin, int rope_T,
                                                             uint16_t* __restrict__ q_out, uint16_t* __restrict__ kv, int64_t ld_kv,
                                                             int32_t* __restrict__ status, int B, int Tmax, int nh, int hd, float sgn) {
  const int dm = nh * hd;
  const int cpr = 3 * dm / 8;  // 16-byte chunks per qkv row
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * cpr) return;
  const int b = (int)(i / cpr);
  const int c = (int)(i - (int64_t)b * cpr);
  const int t = pos[b];
  const int lim = Tmax < rope_T ? Tmax : rope_T;
  if (t < 0 || t >= lim) {  // nothing is written for this sequence
    if (c == 0) status[0] = 1;
    return;
  }
  const int col = c * 8;
  bf16x8_t v = ld_bf16x8(qkv + (int64_t)b * ld_qkv + col);
  if (col < 2 * dm) {  // q | k: the rotation of rope_qk_kernel (attn.hip), same table loads, same rope8
    const int pair0 = (col % hd) / 2;
    const f32x4_t cs = *reinterpret_cast<const f32x4_t*>(rcos + (int64_t)t * (hd / 2) + pair0);
    const f32x4_t sn = *reinterpret_cast<const f32x4_t*>(rsin + (int64_t)t * (hd / 2) + pair0);
    v = rope8(v, cs, sn, sgn);
  }
  if (col < dm)
    st_bf16x8(q_out + (int64_t)b * dm + col, v);
  else
    st_bf16x8(kv + ((int64_t)b * Tmax + t) * ld_kv + (col - dm), v);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plm_attn_decode
// ---------------------------------------------------------------------------------------------------------------------------------
// exp2(x - m) with the one hazard of an online softmax taken out: when nothing has been seen yet m is -inf and x may be too
// (-inf - -inf = NaN); subtracting 0 instead gives exp2(-inf) = 0, which is the right weight of an empty partial
__device__ __forceinline__ float dec_base(float m) { return m == -INFINITY ? 0.f : m; }

// Workspace: ml fp32 [B*nh, S, 2] (running maximum in log2 units, sum of 2^(s - m)) then acc fp32 [B*nh, S, hd] (sum of 2^(s - m) v).
template <int HD>
__global__ __launch_bounds__(DEC_THREADS) void attn_decode_split_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ kv,
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
  const uint16_t* kbase = kv + (int64_t)b * Tmax * ld_kv + h * HD + sub * 8;  // + j * ld_kv: k of key j; + dm: its v

  float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;

  for (int j0 = k0 + wave * (KPW * DEC_UNROLL); j0 < k1; j0 += DEC_WAVES * KPW * DEC_UNROLL) {
    bf16x8_t kk[DEC_UNROLL], vv[DEC_UNROLL];
    bool ok[DEC_UNROLL];
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {  // all loads first: the kernel lives on memory-level parallelism
      const int j = j0 + u * KPW + grp;
      ok[u] = j < k1;
      kk[u] = zero_bf16x8();
      vv[u] = zero_bf16x8();
      if (ok[u]) {  // rows at and beyond lens[b] are never read (they may hold anything, and j may be past Tmax)
        const uint16_t* p = kbase + (int64_t)j * ld_kv;
        kk[u] = ld_bf16x8(p);
        vv[u] = ld_bf16x8(p + dm);
      }
    }
#pragma unroll
    for (int u = 0; u < DEC_UNROLL; ++u) {
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d = fmaf(qf[e], bf2f(kk[u][e]), d);
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, PLM_WAVE);  // inside the lane group
      const float sc = ok[u] ? d : -INFINITY;
      const float mn = fmaxf(m, sc);
      const float base = dec_base(mn);
      const float alpha = __builtin_amdgcn_exp2f(m - base);
      const float p = __builtin_amdgcn_exp2f(sc - base);
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

// one workgroup of HD threads per (sequence, head): the S partials in split order
template <int HD>
__global__ __launch_bounds__(HD) void attn_decode_combine_kernel(const float* __restrict__ ws_ml, const float* __restrict__ ws_acc,
                                                                 uint16_t* __restrict__ out, float* __restrict__ lse, int S) {
  const int bh = blockIdx.x, d = threadIdx.x;
  const float* ml = ws_ml + (int64_t)bh * S * 2;
  float mm = -INFINITY;
  for (int s = 0; s < S; ++s) mm = fmaxf(mm, ml[2 * s]);
  bf16_t o = f2bf(0.f);
  float L = INFINITY;  // no key at all (lens[b] == 0): the masked kernels' rule for such a row, out = 0 and lse = +inf
  if (mm != -INFINITY) {
    float ll = 0.f, a = 0.f;
    for (int s = 0; s < S; ++s) {
      const float ms = ml[2 * s];
      if (ms == -INFINITY) continue;  // an empty split carries no weight
      const float sc = __builtin_amdgcn_exp2f(ms - mm);
      ll += ml[2 * s + 1] * sc;
      a += ws_acc[((int64_t)bh * S + s) * HD + d] * sc;
    }
    o = f2bf(a / ll);
    L = mm + __builtin_amdgcn_logf(ll);  // base-2 LSE, plm_attn_fwd's convention
  }
  reinterpret_cast<bf16_t*>(out)[(int64_t)bh * HD + d] = o;
  if (lse != nullptr && d == 0) lse[bh] = L;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------------------
// splits == 0: enough workgroups for two per CU, but no split shorter than 64 keys of the longest possible sequence.  A function of
// B, nh, Tmax and the CU count alone: what lens holds on the device is never consulted.
static int dec_resolve_splits(int64_t B, int64_t nh, int64_t Tmax, int splits) {
  if (splits != 0) return splits;
  int64_t s = plm_cdiv(2 * DEC_CUS, B * nh);
  const int64_t cap = plm_cdiv(Tmax, 64);
  if (s > cap) s = cap;
  if (s > DEC_MAX_SPLITS) s = DEC_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

static bool dec_shape_ok(int64_t B, int64_t nh, int64_t hd, int64_t Tmax) {
  return B > 0 && nh > 0 && Tmax > 0 && B < 65536 && nh < 65536 && Tmax < (1 << 24) && B * nh < ((int64_t)1 << 31) &&
         (hd == 32 || hd == 64 || hd == 128);
}

static size_t dec_ws_bytes(int64_t B, int64_t nh, int64_t hd, int S) {
  const size_t parts = (size_t)B * (size_t)nh * (size_t)S;
  return (parts * (2 + (size_t)hd) * sizeof(float) + 15) / 16 * 16;
}

extern "C" size_t plm_attn_decode_workspace_bytes(int64_t B, int64_t nh, int64_t hd, int64_t Tmax, int splits) {
  if (!dec_shape_ok(B, nh, hd, Tmax) || splits < 0 || splits > DEC_MAX_SPLITS) return 0;
  return dec_ws_bytes(B, nh, hd, dec_resolve_splits(B, nh, Tmax, splits));
}

extern "C" int plm_kv_append_rope(const uint16_t* qkv, int64_t ld_qkv, const int32_t* pos, const float* rope_cos, const float* rope_sin,
                                  int64_t rope_T, uint16_t* q_out, uint16_t* kv, int64_t ld_kv, int32_t* status, int64_t B, int64_t Tmax,
                                  int64_t nh, int64_t hd, void* stream) {
  PLM_REQUIRE(qkv && pos && rope_cos && rope_sin && q_out && kv && status, "plm_kv_append_rope: null pointer");
  PLM_REQUIRE(hd == 32 || hd == 64 || hd == 128, "plm_kv_append_rope: head_dim %ld unsupported (32, 64, 128)", (long)hd);
  PLM_REQUIRE(dec_shape_ok(B, nh, hd, Tmax) && rope_T > 0 && rope_T < (1 << 24), "plm_kv_append_rope: bad shape B=%ld Tmax=%ld nh=%ld rope_T=%ld",
              (long)B, (long)Tmax, (long)nh, (long)rope_T);
  PLM_REQUIRE(ld_qkv >= 3 * nh * hd && ld_qkv % 8 == 0 && ld_kv >= 2 * nh * hd && ld_kv % 8 == 0,
              "plm_kv_append_rope: row strides must be multiples of 8 and at least 3*nh*hd (qkv) / 2*nh*hd (kv)");
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(q_out) | reinterpret_cast<uintptr_t>(kv) |
                reinterpret_cast<uintptr_t>(rope_cos) | reinterpret_cast<uintptr_t>(rope_sin)) & 15) == 0,
              "plm_kv_append_rope: qkv, q_out, kv and the RoPE tables must be 16-byte aligned");
  const int64_t items = B * (3 * nh * hd / 8);
  hipLaunchKernelGGL(kv_append_rope_kernel, dim3((unsigned)plm_cdiv(items, 256)), dim3(256), 0, (hipStream_t)stream, qkv, ld_qkv, pos, rope_cos,
                     rope_sin, (int)rope_T, q_out, kv, ld_kv, status, (int)B, (int)Tmax, (int)nh, (int)hd, 1.f);
  PLM_CHECK_LAUNCH("plm_kv_append_rope");
  return PLM_OK;
}

template <int HD>
static void dec_launch(const uint16_t* q, const uint16_t* kv, int64_t ld_kv, const int32_t* lens, uint16_t* out, float* lse, int64_t B,
                       int64_t Tmax, int64_t nh, int S, float* ws, hipStream_t s) {
  float* ws_ml = ws;
  float* ws_acc = ws + (size_t)B * nh * S * 2;
  const float c2 = (1.f / sqrtf((float)HD)) * DEC_LOG2E;
  hipLaunchKernelGGL(attn_decode_split_kernel<HD>, dim3((unsigned)(B * nh), (unsigned)S), dim3(DEC_THREADS), 0, s, q, kv, ld_kv, lens, ws_ml,
                     ws_acc, (int)Tmax, (int)nh, S, c2);
  hipLaunchKernelGGL(attn_decode_combine_kernel<HD>, dim3((unsigned)(B * nh)), dim3(HD), 0, s, ws_ml, ws_acc, out, lse, S);
}

extern "C" int plm_attn_decode(const uint16_t* q, const uint16_t* kv, int64_t ld_kv, const int32_t* lens, uint16_t* out, float* lse, int64_t B,
                               int64_t Tmax, int64_t nh, int64_t hd, int splits, void* workspace, size_t workspace_bytes, void* stream) {
  PLM_REQUIRE(q && kv && lens && out && workspace, "plm_attn_decode: null pointer");
  PLM_REQUIRE(hd == 32 || hd == 64 || hd == 128, "plm_attn_decode: head_dim %ld unsupported (32, 64, 128)", (long)hd);
  PLM_REQUIRE(dec_shape_ok(B, nh, hd, Tmax), "plm_attn_decode: bad shape B=%ld Tmax=%ld nh=%ld", (long)B, (long)Tmax, (long)nh);
  PLM_REQUIRE(ld_kv >= 2 * nh * hd && ld_kv % 8 == 0, "plm_attn_decode: the cache's row stride must be a multiple of 8 and at least 2*nh*hd");
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(kv) | reinterpret_cast<uintptr_t>(out) |
                reinterpret_cast<uintptr_t>(workspace)) & 15) == 0,
              "plm_attn_decode: q, kv, out and the workspace must be 16-byte aligned");
  PLM_REQUIRE(splits >= 0 && splits <= DEC_MAX_SPLITS, "plm_attn_decode: splits=%d out of range (0 = automatic, 1..%d forced)", splits,
              DEC_MAX_SPLITS);
  const int S = dec_resolve_splits(B, nh, Tmax, splits);
  const size_t need = dec_ws_bytes(B, nh, hd, S);
  if (workspace_bytes < need) {
    plm_set_error("plm_attn_decode: workspace of %zu bytes required, %zu given", need, workspace_bytes);
    return PLM_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  if (hd == 32) dec_launch<32>(q, kv, ld_kv, lens, out, lse, B, Tmax, nh, S, ws, s);
  else if (hd == 64) dec_launch<64>(q, kv, ld_kv, lens, out, lse, B, Tmax, nh, S, ws, s);
  else dec_launch<128>(q, kv, ld_kv, lens, out, lse, B, Tmax, nh, S, ws, s);
  PLM_CHECK_LAUNCH("plm_attn_decode");
  return PLM_OK;
}
