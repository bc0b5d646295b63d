// Muon for the block matrices: the batched NT GEMM that carries the Newton-Schulz products of a whole list of
// matrices in one launch, and the three calls of the tail around it - prepare (momentum, norm, X0), orthogonalize (steps x 3 batched
// launches) and apply (the update on the shadow tile walk, which writes W, bf16(W) and bf16(W)^T in one pass).
#include <string.h>

#include <vector>

#include "plm_device.h"
#include "plm_shadow_tile.h"

// torch.lerp's two-sided form, as optim.hip spells it (lerp_elem there; the two files are separate translation units)
__device__ __forceinline__ float muon_lerp(float a, float b, float w) {
  const float d = __fsub_rn(b, a);
  return fabsf(w) < 0.5f ? __fmaf_rn(w, d, a) : __fmaf_rn(-d, __fsub_rn(1.f, w), b);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Batched NT GEMM.  Tile body: the 128 x 128 x 64 register-staged body of gemm_nt_kernel (gemm.hip) - the one body in this tree that
// takes every edge (M, N and K tails are zero-filled on the way into LDS), which the problem lists here need: K = 24 or 40 is a legal
// problem.  A workgroup finds its (problem, tile) in a prefix table that travels in the kernel arguments, PLM_NT_BATCH_GROUP problems
// per launch (2.7 KB of the 4 KB a launch may carry).  The epilogue forms fmaf(alpha, acc, beta * d) in fp32, rounds once, stores C
// from the registers and, for the transposed copy, turns the tile in LDS so that Ct leaves as 16-byte row segments as well.
// ---------------------------------------------------------------------------------------------------------------------------------
#define NTB_BM 128
#define NTB_BN 128
#define NTB_BK 64
#define NTB_T_STRIDE 136  // bf16 per row of the transposed tile: 128 + 8 (272 B: 16-byte aligned rows)

struct NtBatchTable {
  const uint16_t* A[PLM_NT_BATCH_GROUP];
  const uint16_t* B[PLM_NT_BATCH_GROUP];
  uint16_t* C[PLM_NT_BATCH_GROUP];
  const uint16_t* D[PLM_NT_BATCH_GROUP];
  uint16_t* Ct[PLM_NT_BATCH_GROUP];
  int lda[PLM_NT_BATCH_GROUP], ldb[PLM_NT_BATCH_GROUP], ldc[PLM_NT_BATCH_GROUP], ldd[PLM_NT_BATCH_GROUP], ldct[PLM_NT_BATCH_GROUP];
  int M[PLM_NT_BATCH_GROUP], N[PLM_NT_BATCH_GROUP], K[PLM_NT_BATCH_GROUP];
  float alpha[PLM_NT_BATCH_GROUP], beta[PLM_NT_BATCH_GROUP];
  int block_base[PLM_NT_BATCH_GROUP + 1];  // first workgroup of each problem; [count] = number of workgroups
  int count;
};

__device__ __forceinline__ int ntb_lds_off(int row, int chunk) {  // byte offset of a 16-byte chunk: gemm.hip's nt_lds_off
  return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

__global__ __launch_bounds__(256) void gemm_nt_batched_kernel(NtBatchTable tb) {
  __shared__ __attribute__((aligned(16))) char smem[NTB_BN * NTB_T_STRIDE * 2];  // 34816 B: the two operand tiles (32 KiB), then the turned C tile
  char* sA = smem;
  char* sB = smem + NTB_BM * NTB_BK * 2;

  int it = 0;
  for (int q = 1; q < tb.count; ++q)
    if ((int)blockIdx.x >= tb.block_base[q]) it = q;  // block-uniform scalar search, as shadow_locate
  const int M = tb.M[it], N = tb.N[it], K = tb.K[it];
  const int local = blockIdx.x - tb.block_base[it];
  const int tiles_n = (N + NTB_BN - 1) / NTB_BN;
  const int m0 = (local / tiles_n) * NTB_BM, n0 = (local % tiles_n) * NTB_BN;
  const uint16_t* __restrict__ A = tb.A[it];
  const uint16_t* __restrict__ B = tb.B[it];
  const int64_t lda = tb.lda[it], ldb = tb.ldb[it];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, hi = lane >> 5;

  // staging assignment: 4 chunks of A and 4 of B per thread
  int ld_row[4], ld_chunk[4];
  const uint16_t* a_ptr[4];
  const uint16_t* b_ptr[4];
  bool a_ok[4], b_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = i * 256 + t;
    ld_row[i] = idx >> 3;
    ld_chunk[i] = idx & 7;
    a_ok[i] = (m0 + ld_row[i]) < M;
    b_ok[i] = (n0 + ld_row[i]) < N;
    a_ptr[i] = A + (int64_t)(m0 + ld_row[i]) * lda + ld_chunk[i] * 8;
    b_ptr[i] = B + (int64_t)(n0 + ld_row[i]) * ldb + ld_chunk[i] * 8;
  }

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  bf16x8_t ra[4], rb[4];
  auto g_load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool kin = (k0 + ld_chunk[i] * 8) < K;  // K % 8 == 0: a chunk is inside or outside as a whole
      ra[i] = (a_ok[i] && kin) ? ld_bf16x8(a_ptr[i] + k0) : zero_bf16x8();
      rb[i] = (b_ok[i] && kin) ? ld_bf16x8(b_ptr[i] + k0) : zero_bf16x8();
    }
  };
  auto s_store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = ntb_lds_off(ld_row[i], ld_chunk[i]);
      *reinterpret_cast<bf16x8_t*>(sA + off) = ra[i];
      *reinterpret_cast<bf16x8_t*>(sB + off) = rb[i];
    }
  };

  const int nk = (K + NTB_BK - 1) / NTB_BK;
  g_load(0);
  s_store();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) g_load((kt + 1) * NTB_BK);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8_t af[2], bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = *reinterpret_cast<const bf16x8_t*>(sA + ntb_lds_off(wm * 64 + i * 32 + l31, ks * 2 + hi));
        bfr[i] = *reinterpret_cast<const bf16x8_t*>(sB + ntb_lds_off(wn * 64 + i * 32 + l31, ks * 2 + hi));
      }
      // D'[n][m] = sum_k B[n][k] A[m][k]: the lane ends up owning one C row (m) and runs of 4 consecutive n
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(bfr[j], af[i], acc[i][j]);
    }
    __syncthreads();  // every read of the operand tiles is done (after the last K-tile: LDS is free for the turned C tile)
    if (kt + 1 < nk) {
      s_store();
      __syncthreads();
    }
  }

  // ---- epilogue: one fp32 expression per element, every rounding spelled out; N % 8 == 0, so a run of 4 is inside or outside as a whole
  const float alpha = tb.alpha[it], beta = tb.beta[it];
  uint16_t* C = tb.C[it];
  const uint16_t* D = tb.D[it];  // may be C itself: an element is read here before this thread writes it
  uint16_t* __restrict__ Ct = tb.Ct[it];
  const int64_t ldc = tb.ldc[it], ldd = tb.ldd[it], ldct = tb.ldct[it];
  bf16_t* sT = reinterpret_cast<bf16_t*>(smem);  // [n local][m local], NTB_T_STRIDE apart
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ml = wm * 64 + i * 32 + l31;
    const int m = m0 + ml;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int nl = wn * 64 + j * 32 + 8 * g + 4 * hi;
        const int n = n0 + nl;
        const bool in = m < M && n < N;
        bf16x4_t o;
        if (D && in) {
          const bf16x4_t d = ld_bf16x4(D + (int64_t)m * ldd + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = f2bf(__fmaf_rn(alpha, acc[i][j][4 * g + e], __fmul_rn(beta, bf2f(d[e]))));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = f2bf(__fmul_rn(alpha, acc[i][j][4 * g + e]));
        }
        if (in) st_bf16x4(C + (int64_t)m * ldc + n, o);
        if (Ct) {
#pragma unroll
          for (int e = 0; e < 4; ++e) sT[(nl + e) * NTB_T_STRIDE + ml] = o[e];
        }
      }
    }
  }
  if (Ct) {  // block-uniform
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int c = q * 256 + t;
      const int nl = c >> 4, mc = (c & 15) * 8;
      const int n = n0 + nl, m = m0 + mc;
      if (n < N && m < M)  // M % 8 == 0: the eight rows are inside together
        st_bf16x8(Ct + (int64_t)n * ldct + m, *reinterpret_cast<const bf16x8_t*>(sT + nl * NTB_T_STRIDE + mc));
    }
  }
}

static bool muon_dim_ok(int64_t v) { return v > 0 && v % 8 == 0 && v < (1ll << 31); }
static bool muon_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// EVERY item is validated before the first launch (the shadow_items_run pattern), then one launch per PLM_NT_BATCH_GROUP problems.
static int nt_batched_run(const char* who, const plm_nt_batch_item* items, int count, hipStream_t stream) {
  PLM_REQUIRE(items && count >= 1, "%s: null pointer or empty list", who);
  int64_t tiles = 0;
  for (int i = 0; i < count; ++i) {
    const plm_nt_batch_item& q = items[i];
    PLM_REQUIRE(q.A && q.B && q.C, "%s: item %d: null A, B or C", who, i);
    PLM_REQUIRE(muon_dim_ok(q.M) && muon_dim_ok(q.N) && muon_dim_ok(q.K), "%s: item %d: M=%ld N=%ld K=%ld must be positive multiples of 8",
                who, i, (long)q.M, (long)q.N, (long)q.K);
    PLM_REQUIRE(muon_dim_ok(q.lda) && muon_dim_ok(q.ldb) && muon_dim_ok(q.ldc) && q.lda >= q.K && q.ldb >= q.K && q.ldc >= q.N,
                "%s: item %d: lda=%ld ldb=%ld ldc=%ld must be multiples of 8 that cover K, K and N", who, i, (long)q.lda, (long)q.ldb, (long)q.ldc);
    PLM_REQUIRE(!q.D || (muon_dim_ok(q.ldd) && q.ldd >= q.N), "%s: item %d: ldd=%ld must be a multiple of 8 >= N", who, i, (long)q.ldd);
    PLM_REQUIRE(!q.Ct || (muon_dim_ok(q.ldct) && q.ldct >= q.M), "%s: item %d: ldct=%ld must be a multiple of 8 >= M", who, i, (long)q.ldct);
    PLM_REQUIRE(muon_aligned(q.A) && muon_aligned(q.B) && muon_aligned(q.C) && muon_aligned(q.D) && muon_aligned(q.Ct),
                "%s: item %d: bases must be 16-byte aligned", who, i);
    if (i % PLM_NT_BATCH_GROUP == 0) tiles = 0;  // the grid of one launch
    tiles += plm_cdiv(q.M, NTB_BM) * plm_cdiv(q.N, NTB_BN);
    PLM_REQUIRE(tiles < (1ll << 31), "%s: too many tiles", who);
  }
  for (int first = 0; first < count; first += PLM_NT_BATCH_GROUP) {
    const int n = count - first < PLM_NT_BATCH_GROUP ? count - first : PLM_NT_BATCH_GROUP;
    NtBatchTable tb{};
    int base = 0;
    for (int i = 0; i < n; ++i) {
      const plm_nt_batch_item& q = items[first + i];
      tb.A[i] = q.A; tb.B[i] = q.B; tb.C[i] = q.C; tb.D[i] = q.D; tb.Ct[i] = q.Ct;
      tb.lda[i] = (int)q.lda; tb.ldb[i] = (int)q.ldb; tb.ldc[i] = (int)q.ldc;
      tb.ldd[i] = q.D ? (int)q.ldd : 0; tb.ldct[i] = q.Ct ? (int)q.ldct : 0;
      tb.M[i] = (int)q.M; tb.N[i] = (int)q.N; tb.K[i] = (int)q.K;
      tb.alpha[i] = q.alpha; tb.beta[i] = q.beta;
      tb.block_base[i] = base;
      base += (int)(plm_cdiv(q.M, NTB_BM) * plm_cdiv(q.N, NTB_BN));
    }
    tb.block_base[n] = base;
    tb.count = n;
    hipLaunchKernelGGL(gemm_nt_batched_kernel, dim3((unsigned)base), dim3(256), 0, stream, tb);
    PLM_CHECK_LAUNCH(who);
  }
  return PLM_OK;
}

extern "C" int plm_gemm_bf16_nt_batched(const plm_nt_batch_item* items, int count, void* stream) {
  return nt_batched_run("plm_gemm_bf16_nt_batched", items, count, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The workspace (layout in include/plainlm_hip.h) and the checks the three calls share
// ---------------------------------------------------------------------------------------------------------------------------------
struct MuonSlots {  // bf16 element offsets of one matrix's blocks from the workspace base
  int64_t x[2], xt[2], a, bm, end;
  int64_t m, n;
};
static MuonSlots muon_slots(int64_t base, int64_t rows, int64_t cols) {
  MuonSlots s;
  s.m = rows < cols ? rows : cols;
  s.n = rows < cols ? cols : rows;
  const int64_t mn = s.m * s.n, mm = s.m * s.m;
  s.x[0] = base; s.xt[0] = base + mn; s.x[1] = base + 2 * mn; s.xt[1] = base + 3 * mn;
  s.a = base + 4 * mn; s.bm = s.a + mm; s.end = s.bm + mm;
  return s;
}
static bool muon_shape_ok(int64_t rows, int64_t cols) { return muon_dim_ok(rows) && muon_dim_ok(cols) && rows * cols < (1ll << 30); }

// bytes of the whole workspace, and the byte offset of the partial sums in *partials; 0 for a refused list
static size_t muon_workspace(const int64_t* rows, const int64_t* cols, int count, size_t* partials) {
  if (!rows || !cols || count < 1) return 0;
  int64_t el = 0, tiles = 0;
  for (int i = 0; i < count; ++i) {
    if (!muon_shape_ok(rows[i], cols[i])) return 0;
    el = muon_slots(el, rows[i], cols[i]).end;
    tiles += plm_cdiv(rows[i], 64) * plm_cdiv(cols[i], 64);
  }
  if (tiles >= (1ll << 31)) return 0;
  if (partials) *partials = (size_t)el * 2;  // el % 8 == 0: 16-byte aligned
  return (size_t)el * 2 + (size_t)plm_cdiv(tiles * 4, 16) * 16;
}

extern "C" size_t plm_muon_workspace_bytes(const int64_t* rows, const int64_t* cols, int count) {
  return muon_workspace(rows, cols, count, nullptr);
}

#define MUON_WORKSPACE(who, need, given, ptr)                                                                     \
  do {                                                                                                            \
    if (!(ptr) || (given) < (need) || !muon_aligned(ptr)) {                                                       \
      plm_set_error("%s: workspace of %zu bytes (16-byte aligned) required, %zu given", who, need, (size_t)(given)); \
      return PLM_E_WORKSPACE;                                                                                     \
    }                                                                                                             \
  } while (0)

// ---------------------------------------------------------------------------------------------------------------------------------
// prepare: launch 1 walks the weights' 64 x 64 tiles (momentum update in place, Ub and Ub^T into the X0 slots through shadow_tile,
// one partial sum per tile); launch 2 sums each matrix's partials in a fixed order and divides X0 | X0t (adjacent, 2 m n elements)
// ---------------------------------------------------------------------------------------------------------------------------------
struct MuonPrepGroup {
  const float* g[PLM_SHADOW_ITEMS_MAX];
  float* buf[PLM_SHADOW_ITEMS_MAX];
  uint16_t* dst[PLM_SHADOW_ITEMS_MAX];    // bf16(U) in the weight's layout: X0 of a wide weight, X0t of a tall one
  uint16_t* dst_t[PLM_SHADOW_ITEMS_MAX];  // its transpose: the other slot
  ShadowTable shape;
};

// fixed-order sum over the workgroup (256 threads): shuffles inside a wave, then the four wave sums in wave order
__device__ __forceinline__ float muon_block_sum(float v) {
  __shared__ float part[4];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return __fadd_rn(__fadd_rn(part[0], part[1]), __fadd_rn(part[2], part[3]));
}

__global__ __launch_bounds__(256) void muon_momentum_kernel(MuonPrepGroup g, float* __restrict__ partials, float momentum, int nesterov,
                                                            const float* __restrict__ clip) {
  int64_t r0, c0;
  const int it = shadow_locate(g.shape, r0, c0);
  const float* __restrict__ G = g.g[it];
  float* __restrict__ Bf = g.buf[it];
  const float cs = clip ? *clip : 1.f;
  const float w1 = 1.f - momentum;
  float sq = 0.f;
  shadow_tile(g.dst[it], g.dst_t[it], g.shape.rows[it], g.shape.cols[it], g.shape.ld_t[it], r0, c0, [&](int64_t o) {
    const f32x4_t gv = *reinterpret_cast<const f32x4_t*>(G + o);
    f32x4_t bv = *reinterpret_cast<const f32x4_t*>(Bf + o), u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
#pragma clang fp contract(off)  // the clipped gradient is rounded before the lerps subtract from it, as clip_grad_norm_ leaves it
      const float gi = __fmul_rn(gv[e], cs);
      bv[e] = muon_lerp(bv[e], gi, w1);
      u[e] = nesterov ? muon_lerp(gi, bv[e], momentum) : bv[e];
      const float ub = bf2f(f2bf(u[e]));  // what shadow_tile stores
      sq = __fmaf_rn(ub, ub, sq);
    }
    *reinterpret_cast<f32x4_t*>(Bf + o) = bv;
    return u;
  });
  const float s = muon_block_sum(sq);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

#define MUON_SCALE_ELEMS 8192  // bf16 elements per workgroup of the division: 256 threads x 4 vectors of 8
struct MuonScaleGroup {
  uint16_t* x[PLM_SHADOW_ITEMS_MAX];   // X0 | X0t
  int numel[PLM_SHADOW_ITEMS_MAX];     // 2 m n
  int part_base[PLM_SHADOW_ITEMS_MAX + 1];  // this matrix's partials (index into the launch's partials)
  int block_base[PLM_SHADOW_ITEMS_MAX + 1];
  int count;
};

__global__ __launch_bounds__(256) void muon_normalize_kernel(MuonScaleGroup g, const float* __restrict__ partials, float* __restrict__ nrm,
                                                             float eps_bf16) {
  int it = 0;
  for (int q = 1; q < g.count; ++q)
    if ((int)blockIdx.x >= g.block_base[q]) it = q;
  const int local = blockIdx.x - g.block_base[it];
  // every workgroup of a matrix forms the same sum in the same order: thread t takes partials t, t + 256, ... ascending
  float s = 0.f;
  for (int i = g.part_base[it] + (int)threadIdx.x; i < g.part_base[it + 1]; i += 256) s = __fadd_rn(s, partials[i]);
  const float total = muon_block_sum(s);
  const float root = bf2f(f2bf(__fsqrt_rn(total)));
  const float nr = root < eps_bf16 ? eps_bf16 : root;  // torch.clamp(min=): a NaN norm stays NaN
  if (local == 0 && threadIdx.x == 0) nrm[it] = nr;
  uint16_t* __restrict__ X = g.x[it];
  const int n = g.numel[it];
#pragma unroll
  for (int q = 0; q < MUON_SCALE_ELEMS / 2048; ++q) {
    const int o = local * MUON_SCALE_ELEMS + (q * 256 + (int)threadIdx.x) * 8;
    if (o < n) {  // numel % 8 == 0
      bf16x8_t v = ld_bf16x8(X + o);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = f2bf(__fdiv_rn(bf2f(v[e]), nr));
      st_bf16x8(X + o, v);
    }
  }
}

static int muon_check_items(const char* who, const plm_muon_item* items, int count, bool prepare) {
  PLM_REQUIRE(items && count >= 1, "%s: null pointer or empty list", who);
  for (int i = 0; i < count; ++i) {
    const plm_muon_item& q = items[i];
    PLM_REQUIRE(muon_shape_ok(q.rows, q.cols), "%s: item %d: rows=%ld cols=%ld must be positive multiples of 8 with rows * cols < 2^30", who, i,
                (long)q.rows, (long)q.cols);
    if (prepare) {
      PLM_REQUIRE(q.g && q.buf, "%s: item %d: null g or buf", who, i);
      PLM_REQUIRE(muon_aligned(q.g) && muon_aligned(q.buf), "%s: item %d: pointers must be 16-byte aligned", who, i);
    } else {
      PLM_REQUIRE(q.p && q.dst && q.dst_t, "%s: item %d: null p, dst or dst_t", who, i);
      PLM_REQUIRE(muon_aligned(q.p) && muon_aligned(q.dst) && muon_aligned(q.dst_t), "%s: item %d: pointers must be 16-byte aligned", who, i);
      PLM_REQUIRE(q.ld_t >= q.rows && muon_dim_ok(q.ld_t), "%s: item %d: ld_t=%ld must be >= rows and a multiple of 8", who, i, (long)q.ld_t);
    }
  }
  return PLM_OK;
}

#define MUON_ITEMS_MAX 4096

static float muon_bf16_round(float f) {  // RNE to bf16 on the host (finite values)
  uint32_t u;
  memcpy(&u, &f, 4);
  u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
  memcpy(&f, &u, 4);
  return f;
}

extern "C" int plm_muon_prepare(const plm_muon_item* items, int count, float momentum, int nesterov, float eps, const float* clip_coef_dev,
                                float* nrm, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "plm_muon_prepare";
  if (const int e = muon_check_items(who, items, count, true)) return e;
  PLM_REQUIRE(count <= MUON_ITEMS_MAX, "%s: %d items, at most %d", who, count, MUON_ITEMS_MAX);
  PLM_REQUIRE(nrm, "%s: null nrm", who);
  PLM_REQUIRE(momentum >= 0.f && momentum < 1.f, "%s: momentum=%g must lie in [0, 1)", who, (double)momentum);
  PLM_REQUIRE(eps >= 0.f, "%s: eps=%g must not be negative", who, (double)eps);
  std::vector<int64_t> rows(count), cols(count);
  for (int i = 0; i < count; ++i) { rows[i] = items[i].rows; cols[i] = items[i].cols; }
  size_t part_off = 0;
  const size_t need = muon_workspace(rows.data(), cols.data(), count, &part_off);
  PLM_REQUIRE(need > 0, "%s: unsupported list", who);
  MUON_WORKSPACE(who, need, workspace_bytes, workspace);
  uint16_t* ws = reinterpret_cast<uint16_t*>(workspace);
  float* partials = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + part_off);
  const float eps_bf16 = muon_bf16_round(eps);  // torch clamps a bf16 norm with the bf16 value of eps

  int64_t el = 0, part = 0;
  for (int first = 0; first < count; first += PLM_SHADOW_ITEMS_MAX) {
    const int n = count - first < PLM_SHADOW_ITEMS_MAX ? count - first : PLM_SHADOW_ITEMS_MAX;
    MuonPrepGroup pg{};
    MuonScaleGroup sg{};
    int base = 0, sbase = 0;
    for (int i = 0; i < n; ++i) {
      const plm_muon_item& q = items[first + i];
      const MuonSlots s = muon_slots(el, q.rows, q.cols);
      el = s.end;
      const bool wide = q.rows <= q.cols;
      pg.g[i] = q.g; pg.buf[i] = q.buf;
      pg.dst[i] = ws + (wide ? s.x[0] : s.xt[0]);
      pg.dst_t[i] = ws + (wide ? s.xt[0] : s.x[0]);
      pg.shape.rows[i] = (int)q.rows; pg.shape.cols[i] = (int)q.cols; pg.shape.ld_t[i] = (int)q.rows;
      pg.shape.block_base[i] = base;
      sg.part_base[i] = base;
      base += (int)(plm_cdiv(q.rows, 64) * plm_cdiv(q.cols, 64));
      sg.x[i] = ws + s.x[0];
      sg.numel[i] = (int)(2 * s.m * s.n);
      sg.block_base[i] = sbase;
      sbase += (int)plm_cdiv(2 * s.m * s.n, MUON_SCALE_ELEMS);
    }
    pg.shape.block_base[n] = base; pg.shape.count = n;
    sg.part_base[n] = base; sg.block_base[n] = sbase; sg.count = n;
    hipLaunchKernelGGL(muon_momentum_kernel, dim3((unsigned)base), dim3(256), 0, (hipStream_t)stream, pg, partials + part, momentum, nesterov,
                       clip_coef_dev);
    PLM_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(muon_normalize_kernel, dim3((unsigned)sbase), dim3(256), 0, (hipStream_t)stream, sg, (const float*)(partials + part),
                       nrm + first, eps_bf16);
    PLM_CHECK_LAUNCH(who);
    part += base;
  }
  return PLM_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// orthogonalize: steps x 3 batched launches over the workspace.  With X^T kept next to X every product is NT:
//   X X^T = nt(X, X) ; A A = nt(A, A) (A is symmetric) ; Bm X = nt(Bm, X^T)
// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int plm_muon_orthogonalize(const int64_t* rows, const int64_t* cols, int count, int steps, float a, float b, float c,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "plm_muon_orthogonalize";
  PLM_REQUIRE(rows && cols && count >= 1, "%s: null pointer or empty list", who);
  PLM_REQUIRE(count <= MUON_ITEMS_MAX, "%s: %d items, at most %d", who, count, MUON_ITEMS_MAX);
  PLM_REQUIRE(steps >= 1 && steps < 100, "%s: steps=%d must lie in 1..99", who, steps);
  const size_t need = muon_workspace(rows, cols, count, nullptr);
  PLM_REQUIRE(need > 0, "%s: rows / cols must be positive multiples of 8 with rows * cols < 2^30", who);
  MUON_WORKSPACE(who, need, workspace_bytes, workspace);
  uint16_t* ws = reinterpret_cast<uint16_t*>(workspace);
  std::vector<plm_nt_batch_item> items(count);
  for (int s = 0; s < steps; ++s) {
    const int cur = s & 1, nxt = cur ^ 1;
    for (int stage = 0; stage < 3; ++stage) {
      int64_t el = 0;
      for (int i = 0; i < count; ++i) {
        const MuonSlots q = muon_slots(el, rows[i], cols[i]);
        el = q.end;
        plm_nt_batch_item& p = items[i];
        p = plm_nt_batch_item{};
        if (stage == 0) {         // A = X X^T
          p.A = ws + q.x[cur]; p.lda = q.n; p.B = p.A; p.ldb = q.n; p.C = ws + q.a; p.ldc = q.m;
          p.M = q.m; p.N = q.m; p.K = q.n; p.alpha = 1.f; p.beta = 0.f;
        } else if (stage == 1) {  // Bm = b A + c (A A)
          p.A = ws + q.a; p.lda = q.m; p.B = p.A; p.ldb = q.m; p.C = ws + q.bm; p.ldc = q.m; p.D = p.A; p.ldd = q.m;
          p.M = q.m; p.N = q.m; p.K = q.m; p.alpha = c; p.beta = b;
        } else {                  // X' = a X + Bm X, and its transpose
          p.A = ws + q.bm; p.lda = q.m; p.B = ws + q.xt[cur]; p.ldb = q.m; p.C = ws + q.x[nxt]; p.ldc = q.n;
          p.D = ws + q.x[cur]; p.ldd = q.n; p.Ct = ws + q.xt[nxt]; p.ldct = q.m;
          p.M = q.m; p.N = q.n; p.K = q.m; p.alpha = 1.f; p.beta = a;
        }
      }
      if (const int e = nt_batched_run(who, items.data(), count, (hipStream_t)stream)) return e;
    }
  }
  return PLM_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// apply: W = fma(-lr_adj, float(O), W * decay) on the shadow tile walk; O is read in the weight's layout
// ---------------------------------------------------------------------------------------------------------------------------------
struct MuonApplyGroup {
  float* p[PLM_SHADOW_ITEMS_MAX];
  const uint16_t* o[PLM_SHADOW_ITEMS_MAX];
  uint16_t* dst[PLM_SHADOW_ITEMS_MAX];
  uint16_t* dst_t[PLM_SHADOW_ITEMS_MAX];
  float lr_adj[PLM_SHADOW_ITEMS_MAX];
  ShadowTable shape;
};

__global__ __launch_bounds__(256) void muon_apply_kernel(MuonApplyGroup g, float decay) {
  int64_t r0, c0;
  const int it = shadow_locate(g.shape, r0, c0);
  float* __restrict__ P = g.p[it];
  const uint16_t* __restrict__ O = g.o[it];
  const float nlr = -g.lr_adj[it];
  shadow_tile(g.dst[it], g.dst_t[it], g.shape.rows[it], g.shape.cols[it], g.shape.ld_t[it], r0, c0, [&](int64_t o) {
    const f32x4_t pv = *reinterpret_cast<const f32x4_t*>(P + o);
    const bf16x4_t ov = ld_bf16x4(O + o);
    f32x4_t pn;
#pragma unroll
    for (int e = 0; e < 4; ++e) pn[e] = __fmaf_rn(nlr, bf2f(ov[e]), __fmul_rn(pv[e], decay));
    *reinterpret_cast<f32x4_t*>(P + o) = pn;
    return pn;
  });
}

extern "C" int plm_muon_apply(const plm_muon_item* items, int count, float decay, int steps, const void* workspace, size_t workspace_bytes,
                              void* stream) {
  const char* who = "plm_muon_apply";
  if (const int e = muon_check_items(who, items, count, false)) return e;
  PLM_REQUIRE(count <= MUON_ITEMS_MAX, "%s: %d items, at most %d", who, count, MUON_ITEMS_MAX);
  PLM_REQUIRE(steps >= 0 && steps < 100, "%s: steps=%d must lie in 0..99", who, steps);
  std::vector<int64_t> rows(count), cols(count);
  for (int i = 0; i < count; ++i) { rows[i] = items[i].rows; cols[i] = items[i].cols; }
  const size_t need = muon_workspace(rows.data(), cols.data(), count, nullptr);
  PLM_REQUIRE(need > 0, "%s: unsupported list", who);
  MUON_WORKSPACE(who, need, workspace_bytes, workspace);
  const uint16_t* ws = reinterpret_cast<const uint16_t*>(workspace);
  int64_t el = 0;
  for (int first = 0; first < count; first += PLM_SHADOW_ITEMS_MAX) {
    const int n = count - first < PLM_SHADOW_ITEMS_MAX ? count - first : PLM_SHADOW_ITEMS_MAX;
    MuonApplyGroup ag{};
    int base = 0;
    for (int i = 0; i < n; ++i) {
      const plm_muon_item& q = items[first + i];
      const MuonSlots s = muon_slots(el, q.rows, q.cols);
      el = s.end;
      ag.p[i] = q.p; ag.dst[i] = q.dst; ag.dst_t[i] = q.dst_t; ag.lr_adj[i] = q.lr_adj;
      ag.o[i] = ws + (q.rows <= q.cols ? s.x[steps & 1] : s.xt[steps & 1]);
      ag.shape.rows[i] = (int)q.rows; ag.shape.cols[i] = (int)q.cols; ag.shape.ld_t[i] = (int)q.ld_t;
      ag.shape.block_base[i] = base;
      base += (int)(plm_cdiv(q.rows, 64) * plm_cdiv(q.cols, 64));
    }
    ag.shape.block_base[n] = base; ag.shape.count = n;
    hipLaunchKernelGGL(muon_apply_kernel, dim3((unsigned)base), dim3(256), 0, (hipStream_t)stream, ag, decay);
    PLM_CHECK_LAUNCH(who);
  }
  return PLM_OK;
}
