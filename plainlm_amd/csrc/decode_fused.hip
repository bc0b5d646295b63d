// The fused layer for gfx950 (DESIGN.md sections 17 and 18): a layer over at most 32 token rows as six plain launches - three skinny-M
// stages around the attention stage's two - issued by ONE library call.  No grid-wide barrier, no flag, no cooperative launch.
//
// The stages share one GEMM core, out[M, N] = A[M, K] W[N, K]^T with 1 <= M <= 32 rows against the bf16 weight shadows, and differ in
// prologue and epilogue.  The rows are B sequences of n chunk rows each, M = B*n, row b*n + r being chunk row r of sequence b:
//   S1r plm_extend_norm_qkv_append_bf16   RMSNorm prologue | w_qkv | RoPE at lens0[b] + r, q to q_out, k | v into the cache row
//                                         (b, lens0[b] + r), under plm_kv_append_rope_rows's contract (ragged chunks by n_new,
//                                         per-sequence refusal, zero q rows)
//   S2  plm_decode_gemm_residual_bf16     bf16 A           | W     | x += float(bf16(.)) on the fp32 residual stream
//   S3  plm_decode_norm_fc1_act_bf16      RMSNorm prologue | w_fc1 | SwiGLU / SiLU / ReLU^2 on the bf16 values
// Every rounding point of the unfused step is kept (bf16 norm output, bf16 GEMM output, RoPE and activation on bf16 values, a bf16 branch
// added to the fp32 stream); only the order of the fp32 sums differs.  S2 and S3 never look at positions.
//
// A decode step is the chunk of one row per sequence, as plm_kv_append_rope is plm_kv_append_rope_rows at n = 1 (attn_cache.hip):
//   S1  plm_decode_norm_qkv_append_bf16   = S1r with n = 1, lens0 = pos, n_new = null: row b rotated at pos[b], its k | v in (b, pos[b])
// the same kernel, the same checks, bit for bit.  So the two layer calls, plm_decode_layer_bf16 and plm_extend_layer_bf16, are one driver
// and differ in their attention stage alone: plm_attn_decode and plm_attn_extend are two kernels, as attn_cache.hip says.
//
// The core.  Each launch streams 1 - 6 MB of weights once against at most 32 rows: a bandwidth and latency problem.  A workgroup of four
// waves owns 16 weight rows (output columns): N / 16 workgroups cover the chip's 256 CUs at the sizes that matter (48 - 256 of them at
// d = 768).  The weights are the A operand of v_mfma_f32_16x16x32_bf16 - lane (i, g) loads 16 bytes of row i at k + 8 g straight from
// global memory, four lanes a 64-byte run of one row, nothing staged - and the activation rows, rounded to bf16 in LDS by the prologue,
// are the B operand: the padded rows of the MFMA cost nothing where the weight stream is the bill, while a VALU product would pay M FMAs
// per weight element and a cross-lane sum per row.  M <= 16 runs one MFMA per K step, M <= 32 two.  K is walked in chunks of KC columns
// (the LDS tile); inside a chunk the four waves take contiguous runs of its 32-wide K steps, every wave loads all its weight fragments of
// the chunk BEFORE the tile is built, so the prologue runs under the loads.  The four waves' partial tiles meet in LDS and are added in
// wave order by the thread that owns the element: no float atomic, nothing depends on arrival order, two runs are bit-equal.
#include "plm_fp8.h"

#define DF_THREADS 256
#define DF_WAVES 4
#define DF_TILE_N 16
#define DF_MAX_ROWS 32
#define DF_PAD 8            // bf16 elements between the rows of the LDS tile (16 bytes: consecutive rows start 4 banks apart)
#define DF_TILE_ELEMS 16640 // 16 x (1024 + 8) = 32 x (512 + 8)

enum { DF_PRO_BF16 = 0, DF_PRO_NORM = 1 };
enum { DF_EPI_RESIDUAL = 1, DF_EPI_GLU = 2, DF_EPI_SILU = 3, DF_EPI_RELU_SQ = 4, DF_EPI_QKV_ROWS = 5, DF_EPI_QKV_ROWS_KV8 = 6 };

struct DfArgs {
  // prologue
  const float* x;        // NORM: the fp32 residual stream [M, K]
  const float* nw;       // NORM: the norm weight [K]
  float eps;
  const uint16_t* a;     // BF16: A [M, K]
  // core
  const uint16_t* w;     // [N, K] bf16, contiguous
  int M, N, K;
  // epilogues
  float* xio;            // RESIDUAL: x [M, N], in place
  uint16_t* out;         // QKV_ROWS: q_out [M, d]; activations: act [M, h]
  uint16_t* kv;          // QKV_ROWS; QKV_ROWS_KV8: the FP8 cache's bytes, ld_kv in bytes
  int64_t ld_kv;
  const float* rcos;
  const float* rsin;
  int32_t* status;
  int rope_T, Tmax, hd, dm, h;
  // QKV_ROWS: row b * n + r is chunk row r of sequence b (a decode step: n = 1, lens0 = the positions)
  int n;
  const int32_t* lens0;  // [M / n]: the cache lengths before the chunk
  const int32_t* n_new;  // [M / n] real rows per chunk, or null: n everywhere
};

// (a, b) -> (a cos - b sin, b cos + a sin): the pair arithmetic of rope8 (plm_device.h) at sgn = +1
__device__ __forceinline__ void df_rope2(bf16_t& a, bf16_t& b, float c, float s) {
  const float af = bf2f(a), bfv = bf2f(b);
  const float sn = s * 1.f;
  a = f2bf(af * c - bfv * sn);
  b = f2bf(bfv * c + af * sn);
}

__device__ __forceinline__ void df_st2(uint16_t* p, bf16_t lo, bf16_t hi) {
  bf16x2_t v;
  v[0] = lo;
  v[1] = hi;
  *reinterpret_cast<bf16x2_t*>(p) = v;
}

template <int PRO, int EPI, bool TWO>
__global__ __launch_bounds__(DF_THREADS) void decode_fused_kernel(const DfArgs p) {
  constexpr int MP = TWO ? 32 : 16;     // rows of the LDS tile
  constexpr int KC = TWO ? 512 : 1024;  // K columns per chunk
  constexpr int PER = KC / 32 / DF_WAVES;  // K steps per wave and chunk
  constexpr int LDX = KC + DF_PAD;
  static_assert(MP * LDX <= DF_TILE_ELEMS, "LDS tile");
  __shared__ __attribute__((aligned(16))) uint16_t s_x[DF_TILE_ELEMS];
  __shared__ __attribute__((aligned(16))) float s_red[DF_WAVES][DF_MAX_ROWS][DF_TILE_N];
  __shared__ float s_rstd[DF_MAX_ROWS];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;
  const int M = p.M, K = p.K;

  // the weight row of this lane: GLU puts 8 gate and 8 up columns of the same 8 outputs into one tile
  int64_t wrow;
  if (EPI == DF_EPI_GLU) wrow = li < 8 ? (int64_t)blockIdx.x * 8 + li : (int64_t)p.h + (int64_t)blockIdx.x * 8 + (li - 8);
  else wrow = (int64_t)blockIdx.x * DF_TILE_N + li;
  const uint16_t* wp = p.w + wrow * K + g * 8;

  if (PRO == DF_PRO_NORM) {  // rstd of every row: one wave per row, lanes over float4 columns, butterfly (plm_rmsnorm_fwd's formula)
    for (int m = wave; m < M; m += DF_WAVES) {
      const float* xr = p.x + (int64_t)m * K;
      float ss = 0.f;
      for (int c = lane; c < (K >> 2); c += 64) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(xr + c * 4);
        ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
      }
      ss = wave_sum(ss);
      if (lane == 0) s_rstd[m] = rsqrtf(ss / (float)K + p.eps);
    }
  }

  f32x4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += KC) {
    const int kc = min(KC, K - k0);
    const int steps = kc >> 5;
    const int per = (steps + DF_WAVES - 1) / DF_WAVES;
    const int s0 = wave * per, s1 = min(steps, s0 + per);
    bf16x8_t wf[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {  // all weight loads of the chunk first
      wf[u] = zero_bf16x8();
      if (s0 + u < s1) wf[u] = ld_bf16x8(wp + k0 + (s0 + u) * 32);
    }
    __syncthreads();  // the previous chunk's reads of the tile are done; s_rstd is visible
    const int vpr = kc >> 2;  // 4-element vectors per row
    for (int idx = tid; idx < MP * vpr; idx += DF_THREADS) {
      const int m = idx / vpr, c = (idx - m * vpr) * 4;
      bf16x4_t o;
      o[0] = o[1] = o[2] = o[3] = f2bf(0.f);
      if (m < M) {
        if (PRO == DF_PRO_NORM) {
          const f32x4_t v = *reinterpret_cast<const f32x4_t*>(p.x + (int64_t)m * K + k0 + c);
          const f32x4_t wv = *reinterpret_cast<const f32x4_t*>(p.nw + k0 + c);
          const float r = s_rstd[m];
          o[0] = f2bf((v[0] * r) * wv[0]);
          o[1] = f2bf((v[1] * r) * wv[1]);
          o[2] = f2bf((v[2] * r) * wv[2]);
          o[3] = f2bf((v[3] * r) * wv[3]);
        } else {
          o = ld_bf16x4(p.a + (int64_t)m * K + k0 + c);
        }
      }
      st_bf16x4(s_x + m * LDX + c, o);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      if (s0 + u < s1) {  // wave-uniform
        const int kk = (s0 + u) * 32 + g * 8;
        acc0 = mfma16(wf[u], ld_bf16x8(s_x + li * LDX + kk), acc0);
        if (TWO) acc1 = mfma16(wf[u], ld_bf16x8(s_x + (li + 16) * LDX + kk), acc1);
      }
    }
  }

  // lane (m = li, g) holds columns 4 g .. 4 g + 3 of rows m and m + 16
  *reinterpret_cast<f32x4_t*>(&s_red[wave][li][4 * g]) = acc0;
  if (TWO) *reinterpret_cast<f32x4_t*>(&s_red[wave][li + 16][4 * g]) = acc1;
  __syncthreads();

  // one thread per (row, adjacent column pair); the four waves' partials in wave order
  const int m = tid >> 3, c2 = (tid & 7) * 2;
  if (m >= M) return;
  float v0 = s_red[0][m][c2], v1 = s_red[0][m][c2 + 1];
#pragma unroll
  for (int w = 1; w < DF_WAVES; ++w) {
    v0 += s_red[w][m][c2];
    v1 += s_red[w][m][c2 + 1];
  }

  if (EPI == DF_EPI_RESIDUAL) {
    float* xo = p.xio + (int64_t)m * p.N + (int64_t)blockIdx.x * DF_TILE_N + c2;
    float2 r = *reinterpret_cast<float2*>(xo);
    r.x += bf2f(f2bf(v0));
    r.y += bf2f(f2bf(v1));
    *reinterpret_cast<float2*>(xo) = r;
  } else if (EPI == DF_EPI_QKV_ROWS || EPI == DF_EPI_QKV_ROWS_KV8) {  // plm_kv_append_rope_rows's contract: row m is chunk row r of sequence b, at position lens0[b] + r
    const int col = blockIdx.x * DF_TILE_N + c2;
    const int dm = p.dm, n = p.n;
    const int b = m / n, r = m - b * n;
    int cb = n;
    if (p.n_new != nullptr) {
      cb = p.n_new[b];
      cb = cb < 0 ? 0 : (cb > n ? n : cb);
    }
    const int l0 = p.lens0[b];
    const int lim = p.Tmax < p.rope_T ? p.Tmax : p.rope_T;
    const bool refused = l0 < 0 || (int64_t)l0 + cb > lim;  // nothing of this sequence is stored
    if (refused && col == 0) p.status[0] = 1;
    if (refused || r >= cb) {  // no cache row; the q row is zeros, so that every byte of q_out is defined
      if (col < dm) df_st2(p.out + (int64_t)m * dm + col, f2bf(0.f), f2bf(0.f));
      return;
    }
    const int t = l0 + r;  // 0 <= t < lim
    bf16_t b0 = f2bf(v0), b1 = f2bf(v1);
    if (col < 2 * dm) {
      const int64_t ti = (int64_t)t * (p.hd / 2) + (col % p.hd) / 2;
      df_rope2(b0, b1, p.rcos[ti], p.rsin[ti]);
    }
    if (col < dm) {
      df_st2(p.out + (int64_t)m * dm + col, b0, b1);
    } else if (EPI == DF_EPI_QKV_ROWS) {
      df_st2(p.kv + ((int64_t)b * p.Tmax + t) * p.ld_kv + (col - dm), b0, b1);
    } else {
      // The FP8 cache.  The 16 columns of this workgroup's tile are one block of the cache row, held as column pairs by the 8 adjacent
      // lanes tid & 7 of this row; all 8 share m, b and r and col >= dm is uniform over the workgroup, so they are here together.  The
      // block maximum is three butterfly steps; the 16 codes meet in the row's first lane, which stores them as one 16-byte vector.
      const float x0 = bf2f(b0), x1 = bf2f(b1);
      float amax = fmaxf(kv8_mag(x0), kv8_mag(x1));
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, PLM_WAVE));
      const unsigned sb = kv8_scale_byte(amax);
      const unsigned pc = kv8_code(x0, amax, sb) | (kv8_code(x1, amax, sb) << 8);  // columns c2, c2 + 1
      const unsigned w = pc | ((unsigned)__shfl_xor((int)pc, 1, PLM_WAVE) << 16);  // even lanes: columns c2 .. c2 + 3
      const int l0g = (tid & 63) & ~7;
      u32x4_t q;
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = (unsigned)__shfl((int)w, l0g + 2 * i, PLM_WAVE);
      if ((tid & 7) == 0) {
        uint8_t* rowp = reinterpret_cast<uint8_t*>(p.kv) + ((int64_t)b * p.Tmax + t) * p.ld_kv;
        const int blk = col - dm;  // the block's first column among the 2 * dm k | v columns
        *reinterpret_cast<u32x4_t*>(rowp + blk) = q;
        rowp[2 * dm + (blk >> 4)] = (uint8_t)sb;
      }
    }
  } else if (EPI == DF_EPI_GLU) {
    if (c2 >= 8) return;  // columns 0..7 of the tile are the gates, 8..15 the ups of the same outputs
    float u0 = s_red[0][m][c2 + 8], u1 = s_red[0][m][c2 + 9];
#pragma unroll
    for (int w = 1; w < DF_WAVES; ++w) {
      u0 += s_red[w][m][c2 + 8];
      u1 += s_red[w][m][c2 + 9];
    }
    df_st2(p.out + (int64_t)m * p.h + (int64_t)blockIdx.x * 8 + c2, plm_swiglu_bf16(f2bf(v0), f2bf(u0)), plm_swiglu_bf16(f2bf(v1), f2bf(u1)));
  } else {
    const float x0 = bf2f(f2bf(v0)), x1 = bf2f(f2bf(v1));
    bf16_t o0, o1;
    if (EPI == DF_EPI_SILU) {
      o0 = f2bf(x0 * plm_sigmoid(x0));
      o1 = f2bf(x1 * plm_sigmoid(x1));
    } else {
      const float r0 = fmaxf(x0, 0.f), r1 = fmaxf(x1, 0.f);
      o0 = f2bf(r0 * r0);
      o1 = f2bf(r1 * r1);
    }
    df_st2(p.out + (int64_t)m * p.h + (int64_t)blockIdx.x * DF_TILE_N + c2, o0, o1);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side: every refusal of a stage is one function, so that the layer driver can run all of them before its first launch
// ---------------------------------------------------------------------------------------------------------------------------------
#define DF_MAX_DIM 65536  // K and N of a stage: far above any model this library serves, keeps every index inside 32 bits

static bool df_aligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr,
                       const void* f = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d) |
           reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(f)) & 15) == 0;
}

static int df_check_rows(const char* fn, int64_t M) {
  PLM_REQUIRE(M >= 1 && M <= DF_MAX_ROWS, "%s: M=%ld rows unsupported (1 <= M <= %d: one decode token per sequence)", fn, (long)M, DF_MAX_ROWS);
  return PLM_OK;
}

// the qkv stage: B sequences of n rows, M = B*n (a decode step: n = 1, lens0 = the positions)
static int df_check_qkv(const char* fn, const float* x, const float* nw, const uint16_t* w_qkv, const int32_t* lens0, const float* rope_cos,
                        const float* rope_sin, int64_t rope_T, const uint16_t* q_out, const uint16_t* kv, int64_t ld_kv, const int32_t* status,
                        int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd, bool kv8 = false) {
  PLM_REQUIRE(x && nw && w_qkv && lens0 && rope_cos && rope_sin && q_out && kv && status, "%s: null pointer", fn);
  PLM_REQUIRE(n >= 1 && n <= DF_MAX_ROWS && B >= 1 && B <= DF_MAX_ROWS && B * n <= DF_MAX_ROWS,
              "%s: B=%ld chunks of n=%ld rows unsupported (n >= 1, 1 <= B*n <= %d rows)", fn, (long)B, (long)n, DF_MAX_ROWS);
  PLM_REQUIRE(hd == 32 || hd == 64 || hd == 128, "%s: head_dim %ld unsupported (32, 64, 128)", fn, (long)hd);
  PLM_REQUIRE(nh > 0 && nh * hd <= DF_MAX_DIM / 4 && Tmax > 0 && Tmax < (1 << 24) && rope_T > 0 && rope_T < (1 << 24),
              "%s: bad shape Tmax=%ld nh=%ld rope_T=%ld", fn, (long)Tmax, (long)nh, (long)rope_T);
  PLM_REQUIRE((nh * hd) % 32 == 0, "%s: d = nh*hd = %ld unsupported (d %% 32 == 0)", fn, (long)(nh * hd));
  if (kv8) PLM_REQUIRE(ld_kv >= kv8_row_payload(nh * hd) && ld_kv % 16 == 0,
                       "%s: the FP8 cache's row stride must be a multiple of 16 bytes and at least 2*nh*hd + nh*hd/8", fn);
  else PLM_REQUIRE(ld_kv >= 2 * nh * hd && ld_kv % 8 == 0, "%s: the cache's row stride must be a multiple of 8 and at least 2*nh*hd", fn);
  PLM_REQUIRE(df_aligned(x, nw, w_qkv, q_out, kv), "%s: x, the norm weight, w_qkv, q_out and kv must be 16-byte aligned", fn);
  return PLM_OK;
}

static int df_check_residual(const char* fn, const float* x, const uint16_t* a, const uint16_t* w, int64_t M, int64_t N, int64_t K) {
  PLM_REQUIRE(x && a && w, "%s: null pointer", fn);
  if (const int e = df_check_rows(fn, M)) return e;
  PLM_REQUIRE(N > 0 && K > 0 && N <= DF_MAX_DIM && K <= DF_MAX_DIM && N % 16 == 0 && K % 32 == 0,
              "%s: unsupported shape N=%ld K=%ld (N %% 16 == 0, K %% 32 == 0, both at most %d)", fn, (long)N, (long)K, DF_MAX_DIM);
  PLM_REQUIRE(df_aligned(x, a, w), "%s: x, A and W must be 16-byte aligned", fn);
  return PLM_OK;
}

static int df_check_fc1(const char* fn, const float* x, const float* nw, const uint16_t* w_fc1, const uint16_t* act, int64_t M, int64_t d,
                        int64_t hidden, int mlp_kind) {
  PLM_REQUIRE(x && nw && w_fc1 && act, "%s: null pointer", fn);
  if (const int e = df_check_rows(fn, M)) return e;
  PLM_REQUIRE(mlp_kind == PLM_DECODE_MLP_GLU || mlp_kind == PLM_DECODE_MLP_SILU || mlp_kind == PLM_DECODE_MLP_RELU_SQ,
              "%s: mlp_kind %d unknown (0 = glu, 1 = silu, 2 = relu_sq)", fn, mlp_kind);
  PLM_REQUIRE(d > 0 && d <= DF_MAX_DIM && d % 32 == 0, "%s: d = %ld unsupported (d %% 32 == 0)", fn, (long)d);
  PLM_REQUIRE(hidden > 0 && hidden <= DF_MAX_DIM / 2 && hidden % 32 == 0, "%s: hidden = %ld unsupported (hidden %% 32 == 0)", fn, (long)hidden);
  PLM_REQUIRE(df_aligned(x, nw, w_fc1, act), "%s: x, the norm weight, w_fc1 and act must be 16-byte aligned", fn);
  return PLM_OK;
}

template <int PRO, int EPI>
static void df_launch(const DfArgs& a, int64_t blocks, hipStream_t s) {
  if (a.M > 16) hipLaunchKernelGGL((decode_fused_kernel<PRO, EPI, true>), dim3((unsigned)blocks), dim3(DF_THREADS), 0, s, a);
  else hipLaunchKernelGGL((decode_fused_kernel<PRO, EPI, false>), dim3((unsigned)blocks), dim3(DF_THREADS), 0, s, a);
}

static void df_launch_qkv(const float* x, const float* nw, float eps, const uint16_t* w_qkv, const int32_t* lens0, const int32_t* n_new,
                          const float* rope_cos, const float* rope_sin, int64_t rope_T, uint16_t* q_out, uint16_t* kv, int64_t ld_kv,
                          int32_t* status, int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd, hipStream_t s, bool kv8 = false) {
  DfArgs a = {};
  const int64_t d = nh * hd;
  a.x = x, a.nw = nw, a.eps = eps, a.w = w_qkv, a.M = (int)(B * n), a.N = (int)(3 * d), a.K = (int)d;
  a.out = q_out, a.kv = kv, a.ld_kv = ld_kv, a.rcos = rope_cos, a.rsin = rope_sin, a.status = status;
  a.rope_T = (int)rope_T, a.Tmax = (int)Tmax, a.hd = (int)hd, a.dm = (int)d;
  a.n = (int)n, a.lens0 = lens0, a.n_new = n_new;
  if (kv8) df_launch<DF_PRO_NORM, DF_EPI_QKV_ROWS_KV8>(a, 3 * d / DF_TILE_N, s);
  else df_launch<DF_PRO_NORM, DF_EPI_QKV_ROWS>(a, 3 * d / DF_TILE_N, s);
}

static void df_launch_residual(float* x, const uint16_t* A, const uint16_t* w, int64_t M, int64_t N, int64_t K, hipStream_t s) {
  DfArgs a = {};
  a.a = A, a.w = w, a.M = (int)M, a.N = (int)N, a.K = (int)K, a.xio = x;
  df_launch<DF_PRO_BF16, DF_EPI_RESIDUAL>(a, N / DF_TILE_N, s);
}

static void df_launch_fc1(const float* x, const float* nw, float eps, const uint16_t* w_fc1, uint16_t* act, int64_t M, int64_t d, int64_t hidden,
                          int mlp_kind, hipStream_t s) {
  DfArgs a = {};
  a.x = x, a.nw = nw, a.eps = eps, a.w = w_fc1, a.M = (int)M, a.K = (int)d, a.out = act, a.h = (int)hidden;
  a.N = (int)(mlp_kind == PLM_DECODE_MLP_GLU ? 2 * hidden : hidden);
  if (mlp_kind == PLM_DECODE_MLP_GLU) df_launch<DF_PRO_NORM, DF_EPI_GLU>(a, hidden / 8, s);
  else if (mlp_kind == PLM_DECODE_MLP_SILU) df_launch<DF_PRO_NORM, DF_EPI_SILU>(a, hidden / DF_TILE_N, s);
  else df_launch<DF_PRO_NORM, DF_EPI_RELU_SQ>(a, hidden / DF_TILE_N, s);
}

extern "C" int plm_decode_norm_qkv_append_bf16(const float* x, const float* norm_w, float eps, const uint16_t* w_qkv, const int32_t* pos,
                                               const float* rope_cos, const float* rope_sin, int64_t rope_T, uint16_t* q_out, uint16_t* kv,
                                               int64_t ld_kv, int32_t* status, int64_t B, int64_t Tmax, int64_t nh, int64_t hd, void* stream) {
  const char* fn = "plm_decode_norm_qkv_append_bf16";
  // one row per sequence at pos[b]: plm_kv_append_rope's way of calling the rows kernel
  if (const int e = df_check_qkv(fn, x, norm_w, w_qkv, pos, rope_cos, rope_sin, rope_T, q_out, kv, ld_kv, status, B, 1, Tmax, nh, hd)) return e;
  df_launch_qkv(x, norm_w, eps, w_qkv, pos, nullptr, rope_cos, rope_sin, rope_T, q_out, kv, ld_kv, status, B, 1, Tmax, nh, hd, (hipStream_t)stream);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" int plm_decode_gemm_residual_bf16(float* x, const uint16_t* A, const uint16_t* W, int64_t M, int64_t N, int64_t K, void* stream) {
  const char* fn = "plm_decode_gemm_residual_bf16";
  if (const int e = df_check_residual(fn, x, A, W, M, N, K)) return e;
  df_launch_residual(x, A, W, M, N, K, (hipStream_t)stream);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" int plm_decode_norm_fc1_act_bf16(const float* x, const float* norm_w, float eps, const uint16_t* w_fc1, uint16_t* act, int64_t M,
                                            int64_t d, int64_t hidden, int mlp_kind, void* stream) {
  const char* fn = "plm_decode_norm_fc1_act_bf16";
  if (const int e = df_check_fc1(fn, x, norm_w, w_fc1, act, M, d, hidden, mlp_kind)) return e;
  df_launch_fc1(x, norm_w, eps, w_fc1, act, M, d, hidden, mlp_kind, (hipStream_t)stream);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" int plm_extend_norm_qkv_append_bf16(const float* x, const float* norm_w, float eps, const uint16_t* w_qkv, const int32_t* lens0,
                                               const int32_t* n_new, const float* rope_cos, const float* rope_sin, int64_t rope_T,
                                               uint16_t* q_out, uint16_t* kv, int64_t ld_kv, int32_t* status, int64_t B, int64_t n, int64_t Tmax,
                                               int64_t nh, int64_t hd, void* stream) {
  const char* fn = "plm_extend_norm_qkv_append_bf16";
  if (const int e = df_check_qkv(fn, x, norm_w, w_qkv, lens0, rope_cos, rope_sin, rope_T, q_out, kv, ld_kv, status, B, n, Tmax, nh, hd)) return e;
  df_launch_qkv(x, norm_w, eps, w_qkv, lens0, n_new, rope_cos, rope_sin, rope_T, q_out, kv, ld_kv, status, B, n, Tmax, nh, hd, (hipStream_t)stream);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

// The attention stage of a layer: what tells the two layer entry points apart.  The decode layer is n = 1 rows per sequence with
// DF_ATTN_DECODE (its per-sequence operands: pos, lens); the extend layer any n with DF_ATTN_EXTEND (lens0, n_new - which may be null).
enum DfAttn { DF_ATTN_DECODE, DF_ATTN_EXTEND };

// Workspace of a layer at M = B*n rows: q bf16 [M, d] | attention output bf16 [M, d] | activation bf16 [M, hidden] | the attention stage's
// partials, every part a multiple of 16 bytes.  A function of the shapes and the splits argument alone.
static size_t df_round16(size_t n) { return (n + 15) / 16 * 16; }

static size_t df_layer_workspace_bytes(DfAttn attn, int64_t B, int64_t n, int64_t nh, int64_t hd, int64_t hidden, int64_t Tmax, int splits) {
  if (B < 1 || B > DF_MAX_ROWS || n < 1 || n > DF_MAX_ROWS || B * n > DF_MAX_ROWS || nh < 1 || nh * hd > DF_MAX_DIM / 4 || (nh * hd) % 32 != 0 ||
      hidden < 1 || hidden > DF_MAX_DIM / 2 || hidden % 32 != 0)
    return 0;
  // 0 for a head_dim, Tmax or splits the attention stage refuses
  const size_t att = attn == DF_ATTN_DECODE ? plm_attn_decode_workspace_bytes(B, nh, hd, Tmax, splits)
                                            : plm_attn_extend_workspace_bytes(B, n, nh, hd, Tmax, splits);
  if (att == 0) return 0;
  const size_t M = (size_t)(B * n), d = (size_t)(nh * hd);
  return 2 * df_round16(M * d * 2) + df_round16(M * (size_t)hidden * 2) + att;
}

extern "C" size_t plm_decode_layer_workspace_bytes(int64_t B, int64_t nh, int64_t hd, int64_t hidden, int64_t Tmax, int splits) {
  return df_layer_workspace_bytes(DF_ATTN_DECODE, B, 1, nh, hd, hidden, Tmax, splits);
}

extern "C" size_t plm_extend_layer_workspace_bytes(int64_t B, int64_t n, int64_t nh, int64_t hd, int64_t hidden, int64_t Tmax, int splits) {
  return df_layer_workspace_bytes(DF_ATTN_EXTEND, B, n, nh, hd, hidden, Tmax, splits);
}

// The layer driver of both entry points: p0 = lens0, the position of every sequence's first row; p1 is the attention stage's own
// per-sequence operand: lens (required) of DF_ATTN_DECODE; n_new (may be null), which the qkv stage takes too, of DF_ATTN_EXTEND.
static int df_layer(const char* fn, DfAttn attn, float* x, const float* attn_norm_w, const float* mlp_norm_w, float eps, const uint16_t* w_qkv,
                    const uint16_t* w_out, const uint16_t* w_fc1, const uint16_t* w_fc2, const int32_t* p0, const int32_t* p1,
                    const float* rope_cos, const float* rope_sin, int64_t rope_T, uint16_t* kv, int64_t ld_kv, int32_t* status, int64_t B, int64_t n,
                    int64_t Tmax, int64_t nh, int64_t hd, int64_t hidden, int mlp_kind, int splits, void* workspace, size_t workspace_bytes,
                    void* stream, bool kv8 = false) {
  PLM_REQUIRE(x && attn_norm_w && mlp_norm_w && w_qkv && w_out && w_fc1 && w_fc2 && p0 && (attn == DF_ATTN_EXTEND || p1) && rope_cos && rope_sin &&
                  kv && status && workspace,
              "%s: null pointer", fn);
  PLM_REQUIRE(df_aligned(workspace), "%s: the workspace must be 16-byte aligned", fn);
  const int64_t d = nh * hd;
  char* ws = static_cast<char*>(workspace);
  // every refusal of every stage before the first launch (the sub-buffers stand in for the stages' own operands)
  uint16_t* q = reinterpret_cast<uint16_t*>(ws);
  if (const int e = df_check_qkv(fn, x, attn_norm_w, w_qkv, p0, rope_cos, rope_sin, rope_T, q, kv, ld_kv, status, B, n, Tmax, nh, hd, kv8)) return e;
  const int64_t M = B * n;
  if (const int e = df_check_residual(fn, x, q, w_out, M, d, d)) return e;
  if (const int e = df_check_fc1(fn, x, mlp_norm_w, w_fc1, q, M, d, hidden, mlp_kind)) return e;
  if (const int e = df_check_residual(fn, x, q, w_fc2, M, d, hidden)) return e;
  PLM_REQUIRE(splits >= 0 && splits <= 64, "%s: splits=%d out of range (0 = automatic, 1..64 forced)", fn, splits);
  // the attention stage's own shape refusals are its workspace query's: 0 for anything plm_attn_decode / plm_attn_extend would refuse
  const size_t need = df_layer_workspace_bytes(attn, B, n, nh, hd, hidden, Tmax, splits);
  PLM_REQUIRE(need != 0, "%s: bad shape B=%ld n=%ld Tmax=%ld nh=%ld hd=%ld hidden=%ld", fn, (long)B, (long)n, (long)Tmax, (long)nh, (long)hd,
              (long)hidden);
  if (workspace_bytes < need) {
    plm_set_error("%s: workspace of %zu bytes required, %zu given", fn, need, workspace_bytes);
    return PLM_E_WORKSPACE;
  }
  const size_t qb = df_round16((size_t)M * (size_t)d * 2), ab = df_round16((size_t)M * (size_t)hidden * 2);
  uint16_t* attn_out = reinterpret_cast<uint16_t*>(ws + qb);
  uint16_t* act = reinterpret_cast<uint16_t*>(ws + 2 * qb);
  void* att = ws + 2 * qb + ab;
  const size_t att_bytes = need - 2 * qb - ab;
  hipStream_t s = (hipStream_t)stream;
  df_launch_qkv(x, attn_norm_w, eps, w_qkv, p0, attn == DF_ATTN_EXTEND ? p1 : nullptr, rope_cos, rope_sin, rope_T, q, kv, ld_kv, status, B, n, Tmax,
                nh, hd, s, kv8);
  const uint8_t* c8 = reinterpret_cast<const uint8_t*>(kv);
  int e;
  if (attn == DF_ATTN_DECODE)
    e = kv8 ? plm_attn_decode_kv8(q, c8, ld_kv, p1, attn_out, nullptr, B, Tmax, nh, hd, splits, att, att_bytes, stream)
            : plm_attn_decode(q, kv, ld_kv, p1, attn_out, nullptr, B, Tmax, nh, hd, splits, att, att_bytes, stream);
  else
    e = kv8 ? plm_attn_extend_kv8(q, c8, ld_kv, p0, p1, attn_out, nullptr, B, n, Tmax, nh, hd, splits, att, att_bytes, stream)
            : plm_attn_extend(q, kv, ld_kv, p0, p1, attn_out, nullptr, B, n, Tmax, nh, hd, splits, att, att_bytes, stream);
  if (e) return e;
  df_launch_residual(x, attn_out, w_out, M, d, d, s);
  df_launch_fc1(x, mlp_norm_w, eps, w_fc1, act, M, d, hidden, mlp_kind, s);
  df_launch_residual(x, act, w_fc2, M, d, hidden, s);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" int plm_decode_layer_bf16(float* x, const float* attn_norm_w, const float* mlp_norm_w, float eps, const uint16_t* w_qkv,
                                     const uint16_t* w_out, const uint16_t* w_fc1, const uint16_t* w_fc2, const int32_t* pos,
                                     const int32_t* lens, const float* rope_cos, const float* rope_sin, int64_t rope_T, uint16_t* kv,
                                     int64_t ld_kv, int32_t* status, int64_t B, int64_t Tmax, int64_t nh, int64_t hd, int64_t hidden,
                                     int mlp_kind, int splits, void* workspace, size_t workspace_bytes, void* stream) {
  return df_layer("plm_decode_layer_bf16", DF_ATTN_DECODE, x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, pos, lens, rope_cos, rope_sin,
                  rope_T, kv, ld_kv, status, B, 1, Tmax, nh, hd, hidden, mlp_kind, splits, workspace, workspace_bytes, stream);
}

extern "C" int plm_extend_layer_bf16(float* x, const float* attn_norm_w, const float* mlp_norm_w, float eps, const uint16_t* w_qkv,
                                     const uint16_t* w_out, const uint16_t* w_fc1, const uint16_t* w_fc2, const int32_t* lens0,
                                     const int32_t* n_new, const float* rope_cos, const float* rope_sin, int64_t rope_T, uint16_t* kv,
                                     int64_t ld_kv, int32_t* status, int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd, int64_t hidden,
                                     int mlp_kind, int splits, void* workspace, size_t workspace_bytes, void* stream) {
  return df_layer("plm_extend_layer_bf16", DF_ATTN_EXTEND, x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lens0, n_new, rope_cos,
                  rope_sin, rope_T, kv, ld_kv, status, B, n, Tmax, nh, hd, hidden, mlp_kind, splits, workspace, workspace_bytes, stream);
}

// ---- the same stage and layers over the FP8 cache: kv8 bytes, ld_kv8 in bytes; everything else as above ----
extern "C" int plm_extend_norm_qkv_append_kv8_bf16(const float* x, const float* norm_w, float eps, const uint16_t* w_qkv, const int32_t* lens0,
                                                   const int32_t* n_new, const float* rope_cos, const float* rope_sin, int64_t rope_T,
                                                   uint16_t* q_out, uint8_t* kv8, int64_t ld_kv8, int32_t* status, int64_t B, int64_t n,
                                                   int64_t Tmax, int64_t nh, int64_t hd, void* stream) {
  const char* fn = "plm_extend_norm_qkv_append_kv8_bf16";
  uint16_t* kv = reinterpret_cast<uint16_t*>(kv8);
  if (const int e = df_check_qkv(fn, x, norm_w, w_qkv, lens0, rope_cos, rope_sin, rope_T, q_out, kv, ld_kv8, status, B, n, Tmax, nh, hd, true)) return e;
  df_launch_qkv(x, norm_w, eps, w_qkv, lens0, n_new, rope_cos, rope_sin, rope_T, q_out, kv, ld_kv8, status, B, n, Tmax, nh, hd, (hipStream_t)stream,
                true);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" int plm_decode_layer_kv8_bf16(float* x, const float* attn_norm_w, const float* mlp_norm_w, float eps, const uint16_t* w_qkv,
                                         const uint16_t* w_out, const uint16_t* w_fc1, const uint16_t* w_fc2, const int32_t* pos,
                                         const int32_t* lens, const float* rope_cos, const float* rope_sin, int64_t rope_T, uint8_t* kv8,
                                         int64_t ld_kv8, int32_t* status, int64_t B, int64_t Tmax, int64_t nh, int64_t hd, int64_t hidden,
                                         int mlp_kind, int splits, void* workspace, size_t workspace_bytes, void* stream) {
  return df_layer("plm_decode_layer_kv8_bf16", DF_ATTN_DECODE, x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, pos, lens, rope_cos,
                  rope_sin, rope_T, reinterpret_cast<uint16_t*>(kv8), ld_kv8, status, B, 1, Tmax, nh, hd, hidden, mlp_kind, splits, workspace,
                  workspace_bytes, stream, true);
}

extern "C" int plm_extend_layer_kv8_bf16(float* x, const float* attn_norm_w, const float* mlp_norm_w, float eps, const uint16_t* w_qkv,
                                         const uint16_t* w_out, const uint16_t* w_fc1, const uint16_t* w_fc2, const int32_t* lens0,
                                         const int32_t* n_new, const float* rope_cos, const float* rope_sin, int64_t rope_T, uint8_t* kv8,
                                         int64_t ld_kv8, int32_t* status, int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd,
                                         int64_t hidden, int mlp_kind, int splits, void* workspace, size_t workspace_bytes, void* stream) {
  return df_layer("plm_extend_layer_kv8_bf16", DF_ATTN_EXTEND, x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lens0, n_new, rope_cos,
                  rope_sin, rope_T, reinterpret_cast<uint16_t*>(kv8), ld_kv8, status, B, n, Tmax, nh, hd, hidden, mlp_kind, splits, workspace,
                  workspace_bytes, stream, true);
}
