// The wide fused layer for gfx950: the ragged paged layer over 1 <= M <= 256 packed rows, six plain launches from
// ONE library call - three wide stages around plm_attn_ragged_paged's two.  The stages are decode_fused.hip's S1 (packed-paged epilogue),
// S2 and S3 with the same rounding points; the core under them is another design, because a workgroup can no longer hold, or afford to
// normalise, every row:
//
//   grid     (N / 16 column tiles) x (ceil(M / RT) row tiles); a workgroup of four waves owns one pair and reads no row outside its tile,
//            rstd included.  RT = 64 gives every wave four v_mfma_f32_16x16x32_bf16 accumulators; RT = 16 and 32 serve M <= 16 and <= 32.
//   operands the weights are the MFMA's A operand, 16 bytes per lane straight from global memory (a row tile re-reads them from L2, at
//            most four times); the activation tile is bf16 in LDS, the B operand, rows WL_PAD elements apart from a power of two.
//   K        walked in chunks of WL_KC = 256 columns; inside a chunk the four waves take contiguous runs of its 32-wide steps (2 / 2 / 2 /
//            2; a tail chunk of s steps ceil(s / 4) each, in wave order).  The loop is software-pipelined: the weight fragments and the
//            raw activation vectors of chunk c + 1 are in flight before the MFMAs of chunk c, and are rounded into the OTHER half of the
//            double-buffered tile after them - one barrier per chunk.
//   LDS      2 x RT x 264 x 2 bytes = 66 KB at RT = 64; the four waves' partial tiles meet in the half the last chunk did not use, so
//            two workgroups share a CU's 160 KB and hide each other's latency where N / 16 is only 48.
//   epilogue one thread per (row, adjacent column pair), RT / 32 pairs each, adds the partials in wave order: no float atomic, two runs
//            are bit-equal.
//
// The bits rule: the partition of K - chunk width, steps per wave, wave order - is a function of K alone.  It never sees M, RT, the
// packing or the grid, and the MFMA computes a row's 16 outputs from that row's B column alone: a row's output depends on that row and
// the weights only, whatever RT served it and whatever else shared the launch.
#include "decode_fused.h"

#define WL_THREADS 256
#define WL_WAVES 4
#define WL_TILE_N 16
#define WL_MAX_ROWS 256
#define WL_KC 256                          // K columns per chunk
#define WL_PER (WL_KC / 32 / WL_WAVES)     // K steps per wave and full chunk
#define WL_PAD 8                           // bf16 elements: consecutive tile rows start 4 banks apart
#define WL_LDX (WL_KC + WL_PAD)

template <int PRO, int EPI, int RT>
__global__ __launch_bounds__(WL_THREADS, 2) void layer_wide_kernel(const DfArgs p) {
  constexpr int NACC = RT / 16;                             // accumulators per wave: 16 rows each
  constexpr int NV = PRO == DF_PRO_NORM ? RT / 4 : RT / 8;  // raw 16-byte activation vectors per thread and chunk
  constexpr int NVF = PRO == DF_PRO_NORM ? NV : 1, NVB = PRO == DF_PRO_NORM ? 1 : NV;
  static_assert(sizeof(float) * WL_WAVES * WL_TILE_N <= sizeof(uint16_t) * WL_LDX, "the partial tiles fit one half of the tile buffer");
  __shared__ __attribute__((aligned(16))) uint16_t s_x[2][RT * WL_LDX];
  __shared__ float s_rstd[RT];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int li = lane & 15, g = lane >> 4;
  const int M = p.M, K = p.K;
  const int m0 = blockIdx.y * RT;  // this workgroup's rows: m0 .. min(M, m0 + RT) - 1

  // the weight row of this lane: GLU puts 8 gate and 8 up columns of the same 8 outputs into one tile
  int64_t wrow;
  if (EPI == DF_EPI_GLU) wrow = li < 8 ? (int64_t)blockIdx.x * 8 + li : (int64_t)p.h + (int64_t)blockIdx.x * 8 + (li - 8);
  else wrow = (int64_t)blockIdx.x * WL_TILE_N + li;
  const uint16_t* wp = p.w + wrow * K + g * 8;

  // The tile's vectors of this thread.  NORM: a wave per row, row wave + 4 i, the lane's four fp32 columns 4 lane (one norm-weight
  // vector serves all its rows); BF16: 32 lanes per row, row (tid >> 5) + 8 i, eight bf16 columns 8 (tid & 31).
  const int vc = PRO == DF_PRO_NORM ? lane * 4 : (tid & 31) * 8;
  const int vr = PRO == DF_PRO_NORM ? wave : tid >> 5;
  constexpr int VRS = PRO == DF_PRO_NORM ? 4 : 8;
  f32x4_t rawf[NVF], nwv = {0.f, 0.f, 0.f, 0.f};
  bf16x8_t rawb[NVB];

  auto load_w = [&](int c, bf16x8_t (&wf)[WL_PER]) {  // the chunk's weight fragments of this wave
    const int k0 = c * WL_KC, steps = min(WL_KC, K - k0) >> 5;
    const int per = (steps + WL_WAVES - 1) / WL_WAVES;
    const int s0 = wave * per, s1 = min(steps, s0 + per);
#pragma unroll
    for (int u = 0; u < WL_PER; ++u) {
      wf[u] = zero_bf16x8();
      if (s0 + u < s1) wf[u] = ld_bf16x8(wp + k0 + (s0 + u) * 32);
    }
  };
  auto load_a = [&](int c) {  // the chunk's raw activation vectors: issued, not yet used
    const int k0 = c * WL_KC, kc = min(WL_KC, K - k0);
    if (PRO == DF_PRO_NORM && vc < kc) nwv = *reinterpret_cast<const f32x4_t*>(p.nw + k0 + vc);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int m = m0 + vr + VRS * i;
      const bool live = m < M && vc < kc;
      if (PRO == DF_PRO_NORM) {
        rawf[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (live) rawf[i] = *reinterpret_cast<const f32x4_t*>(p.x + (int64_t)m * K + k0 + vc);
      } else {
        rawb[i] = zero_bf16x8();
        if (live) rawb[i] = ld_bf16x8(p.a + (int64_t)m * K + k0 + vc);
      }
    }
  };
  auto store_a = [&](int c, uint16_t* buf) {  // rounded into the tile: (x rstd) w as plm_rmsnorm_fwd rounds it; rows past M are zeros
    const int kc = min(WL_KC, K - c * WL_KC);
    if (vc >= kc) return;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int r = vr + VRS * i;
      if (PRO == DF_PRO_NORM) {
        const float rs = m0 + r < M ? s_rstd[r] : 0.f;
        bf16x4_t o;
        o[0] = f2bf((rawf[i][0] * rs) * nwv[0]);
        o[1] = f2bf((rawf[i][1] * rs) * nwv[1]);
        o[2] = f2bf((rawf[i][2] * rs) * nwv[2]);
        o[3] = f2bf((rawf[i][3] * rs) * nwv[3]);
        st_bf16x4(buf + r * WL_LDX + vc, o);
      } else {
        st_bf16x8(buf + r * WL_LDX + vc, rawb[i]);
      }
    }
  };

  bf16x8_t wf[WL_PER], wfn[WL_PER];
  load_w(0, wf);
  load_a(0);
  if (PRO == DF_PRO_NORM) {  // rstd of this tile's rows only: one wave per row, lanes over float4 columns, butterfly (plm_rmsnorm_fwd's formula)
    for (int r = wave; r < RT && m0 + r < M; r += WL_WAVES) {
      const float* xr = p.x + (int64_t)(m0 + r) * K;
      float ss = 0.f;
      for (int c = lane; c < (K >> 2); c += 64) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(xr + c * 4);
        ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
      }
      ss = wave_sum(ss);
      if (lane == 0) s_rstd[r] = rsqrtf(ss / (float)K + p.eps);
    }
    __syncthreads();
  }
  store_a(0, s_x[0]);

  f32x4_t acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; ++a) acc[a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int nc = (K + WL_KC - 1) / WL_KC;
  for (int c = 0; c < nc; ++c) {
    const bool more = c + 1 < nc;
    if (more) {  // chunk c + 1 is in flight under chunk c's MFMAs
      load_w(c + 1, wfn);
      load_a(c + 1);
    }
    __syncthreads();  // tile c is whole; every read of the other half (chunk c - 1) is done
    const uint16_t* buf = s_x[c & 1];
    const int steps = min(WL_KC, K - c * WL_KC) >> 5;
    const int per = (steps + WL_WAVES - 1) / WL_WAVES;
    const int s0 = wave * per, s1 = min(steps, s0 + per);
#pragma unroll
    for (int u = 0; u < WL_PER; ++u) {
      if (s0 + u < s1) {  // wave-uniform
        const int kk = (s0 + u) * 32 + g * 8;
#pragma unroll
        for (int a = 0; a < NACC; ++a) acc[a] = mfma16(wf[u], ld_bf16x8(buf + (li + 16 * a) * WL_LDX + kk), acc[a]);
      }
    }
    if (more) {
      store_a(c + 1, s_x[(c + 1) & 1]);
#pragma unroll
      for (int u = 0; u < WL_PER; ++u) wf[u] = wfn[u];
    }
  }

  // The partials meet in the half that chunk nc - 1 did not use: its last readers (chunk nc - 2) are behind the last barrier.
  // Lane (m = li, g) holds columns 4 g .. 4 g + 3 of rows m + 16 a.
  float* s_red = reinterpret_cast<float*>(s_x[nc & 1]);  // [WL_WAVES][RT][WL_TILE_N]
#pragma unroll
  for (int a = 0; a < NACC; ++a) *reinterpret_cast<f32x4_t*>(s_red + ((wave * RT + li + 16 * a) * WL_TILE_N + 4 * g)) = acc[a];
  __syncthreads();

  // one thread per (row, adjacent column pair), RT / 32 pairs each; the four waves' partials in wave order
  for (int e = tid; e < RT * 8; e += WL_THREADS) {
    const int ml = e >> 3, c2 = (e & 7) * 2;
    const int m = m0 + ml;
    if (m >= M) continue;
    float v0 = s_red[ml * WL_TILE_N + c2], v1 = s_red[ml * WL_TILE_N + c2 + 1];
#pragma unroll
    for (int w = 1; w < WL_WAVES; ++w) {
      v0 += s_red[(w * RT + ml) * WL_TILE_N + c2];
      v1 += s_red[(w * RT + ml) * WL_TILE_N + c2 + 1];
    }

    if (EPI == DF_EPI_RESIDUAL) {
      float* xo = p.xio + (int64_t)m * p.N + (int64_t)blockIdx.x * WL_TILE_N + c2;
      float2 r = *reinterpret_cast<float2*>(xo);
      r.x += bf2f(f2bf(v0));
      r.y += bf2f(f2bf(v1));
      *reinterpret_cast<float2*>(xo) = r;
    } else if (EPI == DF_EPI_QKV_PACKED_PAGED) {  // plm_kv_paged_append_rope_packed's contract, as decode_fused.hip's epilogue of this name
      const int col = blockIdx.x * WL_TILE_N + c2;
      const int dm = p.dm;
      const int b = p.row_seq[m];
      bool refused = (unsigned)b >= (unsigned)p.B || p.cu_rows[b] > m || m >= p.cu_rows[b + 1];  // padding: nothing stored, nothing reported
      int t = 0;
      if (!refused) {
        const int r = m - p.cu_rows[b];  // 0 <= r <= m < 256
        const int cb = (int)min((int64_t)p.cu_rows[b + 1] - p.cu_rows[b], (int64_t)WL_MAX_ROWS);  // r < cb; more rows than a launch has: inconsistent
        const int l0 = p.lens0[b];
        refused = l0 < 0 || (int64_t)l0 + cb > p.Tmax || (int64_t)l0 + cb > p.rope_T;
        if (!refused) {  // every page the chunk touches: up to 5 at 256 rows (l0 + cb <= Tmax = max_pages * 64: the entries exist)
          const int32_t* trow = p.table + (int64_t)b * p.max_pages;
          for (int pi = l0 / PLM_KV_PAGE_ROWS; pi <= (l0 + cb - 1) / PLM_KV_PAGE_ROWS; ++pi) refused = refused || (unsigned)trow[pi] >= (unsigned)p.n_pages;
        }
        if (refused && col == 0) p.status[0] = 1;
        t = l0 + r;
      }
      if (refused) {
        if (col < dm) df_st2(p.out + (int64_t)m * dm + col, f2bf(0.f), f2bf(0.f));
        continue;
      }
      bf16_t b0 = f2bf(v0), b1 = f2bf(v1);
      if (col < 2 * dm) {
        const int64_t ti = (int64_t)t * (p.hd / 2) + (col % p.hd) / 2;
        df_rope2(b0, b1, p.rcos[ti], p.rsin[ti]);
      }
      if (col < dm) {
        df_st2(p.out + (int64_t)m * dm + col, b0, b1);
      } else {
        const int page = p.table[(int64_t)b * p.max_pages + t / PLM_KV_PAGE_ROWS];  // checked above: 0 <= page < n_pages
        df_st2(p.kv + ((int64_t)page * PLM_KV_PAGE_ROWS + t % PLM_KV_PAGE_ROWS) * p.ld_kv + (col - dm), b0, b1);
      }
    } else if (EPI == DF_EPI_GLU) {
      if (c2 >= 8) continue;  // columns 0..7 of the tile are the gates, 8..15 the ups of the same outputs
      float u0 = s_red[ml * WL_TILE_N + c2 + 8], u1 = s_red[ml * WL_TILE_N + c2 + 9];
#pragma unroll
      for (int w = 1; w < WL_WAVES; ++w) {
        u0 += s_red[(w * RT + ml) * WL_TILE_N + c2 + 8];
        u1 += s_red[(w * RT + ml) * WL_TILE_N + c2 + 9];
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
      df_st2(p.out + (int64_t)m * p.h + (int64_t)blockIdx.x * WL_TILE_N + c2, o0, o1);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host side: every refusal of a stage is one function, so that the layer driver can run all of them before its first launch
// ---------------------------------------------------------------------------------------------------------------------------------
static int wl_check_rows(const char* fn, int64_t M) {
  PLM_REQUIRE(M >= 1 && M <= WL_MAX_ROWS, "%s: M=%ld rows unsupported (1 <= M <= %d packed rows)", fn, (long)M, WL_MAX_ROWS);
  return PLM_OK;
}

static int wl_check_qkv(const char* fn, const float* x, const float* nw, const uint16_t* w_qkv, const int32_t* lens0, const float* rope_cos,
                        const float* rope_sin, int64_t rope_T, const uint16_t* q_out, const uint16_t* kv, int64_t ld_kv, const int32_t* status,
                        int64_t R, int64_t Tmax, int64_t nh, int64_t hd) {
  PLM_REQUIRE(x && nw && w_qkv && lens0 && rope_cos && rope_sin && q_out && kv && status, "%s: null pointer", fn);
  if (const int e = wl_check_rows(fn, R)) return e;
  PLM_REQUIRE(hd == 32 || hd == 64 || hd == 128, "%s: head_dim %ld unsupported (32, 64, 128)", fn, (long)hd);
  PLM_REQUIRE(nh > 0 && nh * hd <= DF_MAX_DIM / 4 && Tmax > 0 && Tmax < (1 << 24) && rope_T > 0 && rope_T < (1 << 24),
              "%s: bad shape Tmax=%ld nh=%ld rope_T=%ld", fn, (long)Tmax, (long)nh, (long)rope_T);
  PLM_REQUIRE((nh * hd) % 32 == 0, "%s: d = nh*hd = %ld unsupported (d %% 32 == 0)", fn, (long)(nh * hd));
  PLM_REQUIRE(ld_kv >= 2 * nh * hd && ld_kv % 8 == 0, "%s: the pool's row stride must be a multiple of 8 and at least 2*nh*hd", fn);
  PLM_REQUIRE(df_aligned(x, nw, w_qkv, q_out, kv), "%s: x, the norm weight, w_qkv, q_out and the pool must be 16-byte aligned", fn);
  return PLM_OK;
}

static int wl_check_residual(const char* fn, const float* x, const uint16_t* a, const uint16_t* w, int64_t M, int64_t N, int64_t K) {
  PLM_REQUIRE(x && a && w, "%s: null pointer", fn);
  if (const int e = wl_check_rows(fn, M)) return e;
  PLM_REQUIRE(N > 0 && K > 0 && N <= DF_MAX_DIM && K <= DF_MAX_DIM && N % 16 == 0 && K % 32 == 0,
              "%s: unsupported shape N=%ld K=%ld (N %% 16 == 0, K %% 32 == 0, both at most %d)", fn, (long)N, (long)K, DF_MAX_DIM);
  PLM_REQUIRE(df_aligned(x, a, w), "%s: x, A and W must be 16-byte aligned", fn);
  return PLM_OK;
}

static int wl_check_fc1(const char* fn, const float* x, const float* nw, const uint16_t* w_fc1, const uint16_t* act, int64_t M, int64_t d,
                        int64_t hidden, int mlp_kind) {
  PLM_REQUIRE(x && nw && w_fc1 && act, "%s: null pointer", fn);
  if (const int e = wl_check_rows(fn, M)) return e;
  PLM_REQUIRE(mlp_kind == PLM_DECODE_MLP_GLU || mlp_kind == PLM_DECODE_MLP_SILU || mlp_kind == PLM_DECODE_MLP_RELU_SQ,
              "%s: mlp_kind %d unknown (0 = glu, 1 = silu, 2 = relu_sq)", fn, mlp_kind);
  PLM_REQUIRE(d > 0 && d <= DF_MAX_DIM && d % 32 == 0, "%s: d = %ld unsupported (d %% 32 == 0)", fn, (long)d);
  PLM_REQUIRE(hidden > 0 && hidden <= DF_MAX_DIM / 2 && hidden % 32 == 0, "%s: hidden = %ld unsupported (hidden %% 32 == 0)", fn, (long)hidden);
  PLM_REQUIRE(df_aligned(x, nw, w_fc1, act), "%s: x, the norm weight, w_fc1 and act must be 16-byte aligned", fn);
  return PLM_OK;
}

// The row tile of a launch: the lowest of 16 / 32 / 64 that holds M, else 64-row tiles.  Under the bits rule it changes no bit.
template <int PRO, int EPI>
static void wl_launch(const DfArgs& a, int64_t col_tiles, hipStream_t s) {
  const unsigned cx = (unsigned)col_tiles;
  if (a.M <= 16) hipLaunchKernelGGL((layer_wide_kernel<PRO, EPI, 16>), dim3(cx, 1), dim3(WL_THREADS), 0, s, a);
  else if (a.M <= 32) hipLaunchKernelGGL((layer_wide_kernel<PRO, EPI, 32>), dim3(cx, 1), dim3(WL_THREADS), 0, s, a);
  else hipLaunchKernelGGL((layer_wide_kernel<PRO, EPI, 64>), dim3(cx, (unsigned)((a.M + 63) / 64)), dim3(WL_THREADS), 0, s, a);
}

static void wl_launch_qkv(const float* x, const float* nw, float eps, const uint16_t* w_qkv, const int32_t* lens0, const float* rope_cos,
                          const float* rope_sin, int64_t rope_T, uint16_t* q_out, uint16_t* pool, int64_t ld_kv, int32_t* status, int64_t R,
                          int64_t nh, int64_t hd, const DfPaged& pg, hipStream_t s) {
  DfArgs a = {};
  const int64_t d = nh * hd;
  a.x = x, a.nw = nw, a.eps = eps, a.w = w_qkv, a.M = (int)R, a.N = (int)(3 * d), a.K = (int)d;
  a.out = q_out, a.kv = pool, a.ld_kv = ld_kv, a.rcos = rope_cos, a.rsin = rope_sin, a.status = status;
  a.rope_T = (int)rope_T, a.Tmax = (int)(pg.max_pages * PLM_KV_PAGE_ROWS), a.hd = (int)hd, a.dm = (int)d;
  a.n = (int)R, a.lens0 = lens0;
  a.table = pg.table, a.max_pages = (int)pg.max_pages, a.n_pages = (int)pg.n_pages;
  a.cu_rows = pg.cu_rows, a.row_seq = pg.row_seq, a.B = (int)pg.B;
  wl_launch<DF_PRO_NORM, DF_EPI_QKV_PACKED_PAGED>(a, 3 * d / WL_TILE_N, s);
}

static void wl_launch_residual(float* x, const uint16_t* A, const uint16_t* w, int64_t M, int64_t N, int64_t K, hipStream_t s) {
  DfArgs a = {};
  a.a = A, a.w = w, a.M = (int)M, a.N = (int)N, a.K = (int)K, a.xio = x;
  wl_launch<DF_PRO_BF16, DF_EPI_RESIDUAL>(a, N / WL_TILE_N, s);
}

static void wl_launch_fc1(const float* x, const float* nw, float eps, const uint16_t* w_fc1, uint16_t* act, int64_t M, int64_t d, int64_t hidden,
                          int mlp_kind, hipStream_t s) {
  DfArgs a = {};
  a.x = x, a.nw = nw, a.eps = eps, a.w = w_fc1, a.M = (int)M, a.K = (int)d, a.out = act, a.h = (int)hidden;
  a.N = (int)(mlp_kind == PLM_DECODE_MLP_GLU ? 2 * hidden : hidden);
  if (mlp_kind == PLM_DECODE_MLP_GLU) wl_launch<DF_PRO_NORM, DF_EPI_GLU>(a, hidden / 8, s);
  else if (mlp_kind == PLM_DECODE_MLP_SILU) wl_launch<DF_PRO_NORM, DF_EPI_SILU>(a, hidden / WL_TILE_N, s);
  else wl_launch<DF_PRO_NORM, DF_EPI_RELU_SQ>(a, hidden / WL_TILE_N, s);
}

extern "C" int plm_wide_gemm_residual_bf16(float* x, const uint16_t* A, const uint16_t* W, int64_t M, int64_t N, int64_t K, void* stream) {
  const char* fn = "plm_wide_gemm_residual_bf16";
  if (const int e = wl_check_residual(fn, x, A, W, M, N, K)) return e;
  wl_launch_residual(x, A, W, M, N, K, (hipStream_t)stream);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" int plm_wide_norm_fc1_act_bf16(const float* x, const float* norm_w, float eps, const uint16_t* w_fc1, uint16_t* act, int64_t M, int64_t d,
                                          int64_t hidden, int mlp_kind, void* stream) {
  const char* fn = "plm_wide_norm_fc1_act_bf16";
  if (const int e = wl_check_fc1(fn, x, norm_w, w_fc1, act, M, d, hidden, mlp_kind)) return e;
  wl_launch_fc1(x, norm_w, eps, w_fc1, act, M, d, hidden, mlp_kind, (hipStream_t)stream);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" int plm_ragged_norm_qkv_append_paged_wide_bf16(const float* x, const float* norm_w, float eps, const uint16_t* w_qkv, const int32_t* lens0,
                                                          const int32_t* cu_rows, const int32_t* row_seq, const float* rope_cos,
                                                          const float* rope_sin, int64_t rope_T, uint16_t* q_out, uint16_t* pool, int64_t ld_kv,
                                                          const int32_t* table, int32_t* status, int64_t R, int64_t B, int64_t max_pages,
                                                          int64_t n_pages, int64_t nh, int64_t hd, void* stream) {
  const char* fn = "plm_ragged_norm_qkv_append_paged_wide_bf16";
  DfPaged pg = {table, nullptr, max_pages, n_pages, 0};
  pg.cu_rows = cu_rows, pg.row_seq = row_seq, pg.R = R, pg.B = B;
  if (const int e = df_check_paged(fn, pg, false)) return e;
  if (const int e = df_check_packed(fn, pg, lens0)) return e;
  if (const int e = wl_check_qkv(fn, x, norm_w, w_qkv, lens0, rope_cos, rope_sin, rope_T, q_out, pool, ld_kv, status, R, max_pages * PLM_KV_PAGE_ROWS,
                                 nh, hd))
    return e;
  wl_launch_qkv(x, norm_w, eps, w_qkv, lens0, rope_cos, rope_sin, rope_T, q_out, pool, ld_kv, status, R, nh, hd, pg, (hipStream_t)stream);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

// The plan of the shared prefixes; key_lo null: the layer attends through plm_attn_ragged_paged
struct WlCascade {
  const int32_t* key_lo;
  const int32_t* tile_rows;
  const int32_t* tile_seq;
  const int32_t* tile_keys;
  int64_t NTg, Pcap;
};

// Workspace of the layer at R rows: q bf16 [R, d] | attention output bf16 [R, d] | activation bf16 [R, hidden] | the attention stage's
// partials, every part a multiple of 16 bytes.  A function of the shapes alone; 0 for a shape the layer refuses.
static size_t wl_layer_bytes(int64_t R, int64_t nh, int64_t hd, int64_t hidden, size_t att) {
  if (R < 1 || R > WL_MAX_ROWS || nh < 1 || nh * hd > DF_MAX_DIM / 4 || (nh * hd) % 32 != 0 || hidden < 1 || hidden > DF_MAX_DIM / 2 || hidden % 32 != 0)
    return 0;
  if (att == 0) return 0;  // a head_dim, Lcap or plan the attention stage refuses
  const size_t d = (size_t)(nh * hd);
  return 2 * df_round16((size_t)R * d * 2) + df_round16((size_t)R * (size_t)hidden * 2) + att;
}

extern "C" size_t plm_ragged_layer_paged_wide_workspace_bytes(int64_t R, int64_t nh, int64_t hd, int64_t hidden, int64_t Lcap) {
  return wl_layer_bytes(R, nh, hd, hidden, plm_attn_ragged_paged_workspace_bytes(R, nh, hd, Lcap));
}

extern "C" size_t plm_ragged_layer_paged_wide_cascade_workspace_bytes(int64_t R, int64_t nh, int64_t hd, int64_t hidden, int64_t Lcap, int64_t NTg,
                                                                      int64_t Pcap) {
  return wl_layer_bytes(R, nh, hd, hidden, plm_attn_ragged_paged_cascade_workspace_bytes(R, nh, hd, Lcap, NTg, Pcap));
}

static int wl_ragged_layer(const char* fn, float* x, const float* attn_norm_w, const float* mlp_norm_w, float eps, const uint16_t* w_qkv,
                           const uint16_t* w_out, const uint16_t* w_fc1, const uint16_t* w_fc2, const int32_t* lens0, const int32_t* cu_rows,
                           const int32_t* row_seq, const float* rope_cos, const float* rope_sin, int64_t rope_T, uint16_t* pool, int64_t ld_kv,
                           const int32_t* table, int32_t* status, int64_t R, int64_t B, int64_t NT, int64_t Lcap, int64_t max_pages,
                           int64_t n_pages, int64_t nh, int64_t hd, int64_t hidden, int mlp_kind, const WlCascade& cs, void* workspace,
                           size_t workspace_bytes, void* stream) {
  PLM_REQUIRE(x && attn_norm_w && mlp_norm_w && w_qkv && w_out && w_fc1 && w_fc2 && lens0 && rope_cos && rope_sin && pool && status && workspace,
              "%s: null pointer", fn);
  PLM_REQUIRE(df_aligned(workspace), "%s: the workspace must be 16-byte aligned", fn);
  DfPaged pg = {table, nullptr, max_pages, n_pages, Lcap};
  pg.cu_rows = cu_rows, pg.row_seq = row_seq, pg.R = R, pg.B = B, pg.NT = NT;
  // every refusal of every stage before the first launch (the workspace's first part stands in for the stages' own operands)
  if (const int e = df_check_paged(fn, pg, true)) return e;
  if (const int e = df_check_packed(fn, pg, lens0)) return e;
  const int64_t d = nh * hd;
  char* ws = static_cast<char*>(workspace);
  uint16_t* q = reinterpret_cast<uint16_t*>(ws);
  if (const int e = wl_check_qkv(fn, x, attn_norm_w, w_qkv, lens0, rope_cos, rope_sin, rope_T, q, pool, ld_kv, status, R, max_pages * PLM_KV_PAGE_ROWS,
                                 nh, hd))
    return e;
  PLM_REQUIRE(NT >= 1 && NT <= R, "%s: NT=%ld tiles outside [1, R = %ld] (a tile holds at least one row)", fn, (long)NT, (long)R);
  if (cs.key_lo) {  // plm_attn_ragged_paged_cascade's own refusals, under this entry point's name
    PLM_REQUIRE(cs.NTg >= 1 && cs.NTg <= R, "%s: NTg=%ld group tiles outside [1, R = %ld] (a tile holds at least one row)", fn, (long)cs.NTg, (long)R);
    PLM_REQUIRE(cs.Pcap >= PLM_KV_PAGE_ROWS && cs.Pcap % PLM_KV_PAGE_ROWS == 0 && cs.Pcap <= max_pages * PLM_KV_PAGE_ROWS,
                "%s: Pcap=%ld is no positive multiple of %d within max_pages * %d = %ld (a prefix is whole pages)", fn, (long)cs.Pcap,
                PLM_KV_PAGE_ROWS, PLM_KV_PAGE_ROWS, (long)(max_pages * PLM_KV_PAGE_ROWS));
    PLM_REQUIRE(((reinterpret_cast<uintptr_t>(cs.key_lo) | reinterpret_cast<uintptr_t>(cs.tile_rows) | reinterpret_cast<uintptr_t>(cs.tile_seq) |
                  reinterpret_cast<uintptr_t>(cs.tile_keys)) & 3) == 0,
                "%s: key_lo, tile_rows, tile_seq and tile_keys must be 4-byte aligned", fn);
  }
  if (const int e = wl_check_residual(fn, x, q, w_out, R, d, d)) return e;
  if (const int e = wl_check_fc1(fn, x, mlp_norm_w, w_fc1, q, R, d, hidden, mlp_kind)) return e;
  if (const int e = wl_check_residual(fn, x, q, w_fc2, R, d, hidden)) return e;
  // the attention stage's own shape refusals are its workspace query's: 0 for anything it would refuse
  const size_t need = cs.key_lo ? plm_ragged_layer_paged_wide_cascade_workspace_bytes(R, nh, hd, hidden, Lcap, cs.NTg, cs.Pcap)
                                : plm_ragged_layer_paged_wide_workspace_bytes(R, nh, hd, hidden, Lcap);
  PLM_REQUIRE(need != 0, "%s: bad shape R=%ld Lcap=%ld nh=%ld hd=%ld hidden=%ld", fn, (long)R, (long)Lcap, (long)nh, (long)hd, (long)hidden);
  if (workspace_bytes < need) {
    plm_set_error("%s: workspace of %zu bytes required, %zu given", fn, need, workspace_bytes);
    return PLM_E_WORKSPACE;
  }
  const size_t qb = df_round16((size_t)R * (size_t)d * 2), ab = df_round16((size_t)R * (size_t)hidden * 2);
  uint16_t* attn_out = reinterpret_cast<uint16_t*>(ws + qb);
  uint16_t* act = reinterpret_cast<uint16_t*>(ws + 2 * qb);
  hipStream_t s = (hipStream_t)stream;
  wl_launch_qkv(x, attn_norm_w, eps, w_qkv, lens0, rope_cos, rope_sin, rope_T, q, pool, ld_kv, status, R, nh, hd, pg, s);
  const int e = cs.key_lo ? plm_attn_ragged_paged_cascade(q, pool, ld_kv, table, lens0, cs.key_lo, cu_rows, row_seq, cs.tile_rows, cs.tile_seq,
                                                          cs.tile_keys, attn_out, nullptr, R, B, NT, cs.NTg, Lcap, cs.Pcap, max_pages, n_pages, nh, hd,
                                                          ws + 2 * qb + ab, need - 2 * qb - ab, stream)
                          : plm_attn_ragged_paged(q, pool, ld_kv, table, lens0, cu_rows, row_seq, attn_out, nullptr, R, B, NT, Lcap, max_pages, n_pages,
                                                  nh, hd, ws + 2 * qb + ab, need - 2 * qb - ab, stream);
  if (e) return e;
  wl_launch_residual(x, attn_out, w_out, R, d, d, s);
  wl_launch_fc1(x, mlp_norm_w, eps, w_fc1, act, R, d, hidden, mlp_kind, s);
  wl_launch_residual(x, act, w_fc2, R, d, hidden, s);
  PLM_CHECK_LAUNCH(fn);
  return PLM_OK;
}

extern "C" int plm_ragged_layer_paged_wide_bf16(float* x, const float* attn_norm_w, const float* mlp_norm_w, float eps, const uint16_t* w_qkv,
                                                const uint16_t* w_out, const uint16_t* w_fc1, const uint16_t* w_fc2, const int32_t* lens0,
                                                const int32_t* cu_rows, const int32_t* row_seq, const float* rope_cos, const float* rope_sin,
                                                int64_t rope_T, uint16_t* pool, int64_t ld_kv, const int32_t* table, int32_t* status, int64_t R,
                                                int64_t B, int64_t NT, int64_t Lcap, int64_t max_pages, int64_t n_pages, int64_t nh, int64_t hd,
                                                int64_t hidden, int mlp_kind, void* workspace, size_t workspace_bytes, void* stream) {
  return wl_ragged_layer("plm_ragged_layer_paged_wide_bf16", x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lens0, cu_rows, row_seq,
                         rope_cos, rope_sin, rope_T, pool, ld_kv, table, status, R, B, NT, Lcap, max_pages, n_pages, nh, hd, hidden, mlp_kind,
                         WlCascade{}, workspace, workspace_bytes, stream);
}

// the wide layer with the cascade attention stage: seven launches
extern "C" int plm_ragged_layer_paged_wide_cascade_bf16(float* x, const float* attn_norm_w, const float* mlp_norm_w, float eps, const uint16_t* w_qkv,
                                                        const uint16_t* w_out, const uint16_t* w_fc1, const uint16_t* w_fc2, const int32_t* lens0,
                                                        const int32_t* key_lo, const int32_t* cu_rows, const int32_t* row_seq,
                                                        const int32_t* tile_rows, const int32_t* tile_seq, const int32_t* tile_keys,
                                                        const float* rope_cos, const float* rope_sin, int64_t rope_T, uint16_t* pool, int64_t ld_kv,
                                                        const int32_t* table, int32_t* status, int64_t R, int64_t B, int64_t NT, int64_t NTg,
                                                        int64_t Lcap, int64_t Pcap, int64_t max_pages, int64_t n_pages, int64_t nh, int64_t hd,
                                                        int64_t hidden, int mlp_kind, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "plm_ragged_layer_paged_wide_cascade_bf16";
  PLM_REQUIRE(key_lo && tile_rows && tile_seq && tile_keys, "%s: null pointer", fn);
  return wl_ragged_layer(fn, x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lens0, cu_rows, row_seq, rope_cos, rope_sin, rope_T, pool,
                         ld_kv, table, status, R, B, NT, Lcap, max_pages, n_pages, nh, hd, hidden, mlp_kind,
                         WlCascade{key_lo, tile_rows, tile_seq, tile_keys, NTg, Pcap}, workspace, workspace_bytes, stream);
}

