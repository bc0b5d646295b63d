// MXFP8 (OCP MX: e4m3fn elements, one E8M0 power-of-two scale per 32 elements): operands and GEMM for the block linears
// (DESIGN.md section 9).
//
//   * plm_mx_quant / plm_mx_quant_multi: bf16 [rows, cols] -> the row-blocked copy ([rows, Kq] bytes + [rows, Kq/32] scales,
//     blocked along cols, Kq = roundup(cols, 128)) and/or the transposed copy ([cols, Kt] + [cols, Kt/32], blocked along rows,
//     Kt = roundup(rows, 128)), in one read of the input.  Padding elements are zero with scale byte 0.
//   * plm_gemm_mx_nt: C[M,N] = deq(A)[M,Kp] . deq(B)[N,Kp]^T on v_mfma_scale_f32_32x32x64_f8f6f4 (2x the bf16 MFMA rate per clock),
//     fp32 accumulation, bf16 store | fp32 store | fp32 accumulate into C.
//
// Scale rule (exact, shared with the CPU reference tests/mx_ref.py): amax = max |x| of the block, E = floor(log2 amax),
// e = E - 8 if amax <= 448 * 2^(E-8) (= 1.75 * 2^E) else E - 7, clamped to [-127, 127]; scale byte e + 127; q = RNE_e4m3fn(x * 2^-e)
// with subnormals.  amax = 0: scale byte 0, zero elements.  Any non-finite element: scale byte 0xFF and every element 0x7F (NaN).
#include "plm_fp8.h"  // mx_e4m3, mx_scale_exp: shared with the FP8 KV cache

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

// ---------------------------------------------------------------------------
// quantizer
// ---------------------------------------------------------------------------
// One block of 32 values: 8 packed dwords (element j in byte j & 3 of dword j >> 2) and the scale byte.
__device__ __forceinline__ unsigned mx_block(const float (&v)[32], unsigned (&q)[8]) {
  float amax = 0.f;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    amax = __builtin_fmaxf(amax, __builtin_fabsf(v[j]));
    bad |= (__float_as_uint(v[j]) & 0x7F800000u) == 0x7F800000u;
  }
  if (bad) {
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = 0x7F7F7F7Fu;
    return 0xFFu;
  }
  if (amax == 0.f) {
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j] = 0u;
    return 0u;
  }
  const int e = mx_scale_exp(amax);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    unsigned w = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) w |= mx_e4m3(__builtin_ldexpf(v[4 * j + i], -e)) << (8 * i);
    q[j] = w;
  }
  return (unsigned)(e + 127);
}

#define PLM_MX_MULTI_MAX 64

struct MxGroup {
  const uint16_t* x[PLM_MX_MULTI_MAX];
  uint8_t* q[PLM_MX_MULTI_MAX];
  uint8_t* s[PLM_MX_MULTI_MAX];
  uint8_t* qt[PLM_MX_MULTI_MAX];
  uint8_t* st[PLM_MX_MULTI_MAX];
  int64_t ld[PLM_MX_MULTI_MAX];
  int rows[PLM_MX_MULTI_MAX];
  int cols[PLM_MX_MULTI_MAX];
  int block_base[PLM_MX_MULTI_MAX + 1];
  int count;
};

// One workgroup = a 32-row x 128-column tile of one item, 128 threads.  Thread t first owns the row block (row t >> 2, columns
// 32 (t & 3) ...+31): it reads those 64 bytes (the tile's only read of the input), writes the row-blocked copy and parks the
// values in LDS; then it owns column t of the tile and writes its 32-row block of the transposed copy.
__global__ __launch_bounds__(128) void mx_quant_kernel(MxGroup g) {
  __shared__ uint16_t tile[32][128 + 2];
  const int bid = blockIdx.x;
  int it = 0;
  while (it + 1 < g.count && bid >= g.block_base[it + 1]) ++it;
  const int local = bid - g.block_base[it];
  const int rows = g.rows[it], cols = g.cols[it];
  const int kq = (cols + 127) & ~127, kt = (rows + 127) & ~127;
  const int tiles_c = kq >> 7;
  const int r0 = (local / tiles_c) * 32, c0 = (local % tiles_c) * 128;
  const int t = threadIdx.x;
  const uint16_t* __restrict__ x = g.x[it];
  uint8_t* __restrict__ q = g.q[it];
  uint8_t* __restrict__ qt = g.qt[it];

  {
    const int r = t >> 2, cb = c0 + 32 * (t & 3);
    const int gr = r0 + r;
    float v[32];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bf16x8_t w = zero_bf16x8();
      if (gr < rows && cb + 8 * i < cols) w = ld_bf16x8(x + (int64_t)gr * g.ld[it] + cb + 8 * i);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[8 * i + j] = bf2f(w[j]);
    }
    if (q && gr < rows) {
      unsigned o[8];
      const unsigned sc = mx_block(v, o);
      u32x4_t* dst = reinterpret_cast<u32x4_t*>(q + (int64_t)gr * kq + cb);
      dst[0] = u32x4_t{o[0], o[1], o[2], o[3]};
      dst[1] = u32x4_t{o[4], o[5], o[6], o[7]};
      g.s[it][(int64_t)gr * (kq >> 5) + (cb >> 5)] = (uint8_t)sc;
    }
    if (qt) {
#pragma unroll
      for (int j = 0; j < 32; ++j) tile[r][32 * (t & 3) + j] = __builtin_bit_cast(uint16_t, f2bf(v[j]));
    }
  }
  if (!qt) return;  // workgroup-uniform
  __syncthreads();
  const int gc = c0 + t;
  if (gc >= cols) return;
  float v[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) v[j] = __uint_as_float((unsigned)tile[j][t] << 16);
  unsigned o[8];
  const unsigned sc = mx_block(v, o);
  u32x4_t* dst = reinterpret_cast<u32x4_t*>(qt + (int64_t)gc * kt + r0);
  dst[0] = u32x4_t{o[0], o[1], o[2], o[3]};
  dst[1] = u32x4_t{o[4], o[5], o[6], o[7]};
  g.st[it][(int64_t)gc * (kt >> 5) + (r0 >> 5)] = (uint8_t)sc;
}

static int mx_check_item(const plm_mx_quant_item& q, const char* who, int idx) {
  PLM_REQUIRE(q.x, "%s: item %d: null input", who, idx);
  PLM_REQUIRE(!q.q == !q.s && !q.qt == !q.st, "%s: item %d: an output pair needs both its data and its scale pointer", who, idx);
  PLM_REQUIRE(q.q || q.qt, "%s: item %d: neither output pair given", who, idx);
  PLM_REQUIRE(q.rows > 0 && q.cols > 0 && q.cols % 8 == 0 && q.rows < (1ll << 30) && q.cols < (1ll << 30),
              "%s: item %d: rows=%ld cols=%ld (need rows > 0, cols > 0 and cols %% 8 == 0)", who, idx, (long)q.rows, (long)q.cols);
  PLM_REQUIRE(q.ld >= q.cols && q.ld % 8 == 0, "%s: item %d: ld=%ld must be >= cols and a multiple of 8", who, idx, (long)q.ld);
  PLM_REQUIRE(((uintptr_t)q.x & 15) == 0 && ((uintptr_t)q.q & 15) == 0 && ((uintptr_t)q.qt & 15) == 0,
              "%s: item %d: x, q and qt must be 16-byte aligned", who, idx);
  const int64_t kq = (q.cols + 127) / 128 * 128, kt = (q.rows + 127) / 128 * 128;
  PLM_REQUIRE((q.rows + 31) / 32 * (kq / 128) < (1ll << 30) && kq * kt > 0, "%s: item %d: too large", who, idx);
  return PLM_OK;
}

extern "C" int plm_mx_quant_multi(const plm_mx_quant_item* items, int count, void* stream) {
  PLM_REQUIRE(items && count >= 1, "plm_mx_quant_multi: null pointer or empty list");
  for (int i = 0; i < count; ++i) {
    const int rc = mx_check_item(items[i], "plm_mx_quant_multi", i);
    if (rc != PLM_OK) return rc;
  }
  for (int first = 0; first < count; first += PLM_MX_MULTI_MAX) {
    const int n = count - first < PLM_MX_MULTI_MAX ? count - first : PLM_MX_MULTI_MAX;
    MxGroup g{};
    int64_t base = 0;
    for (int i = 0; i < n; ++i) {
      const plm_mx_quant_item& q = items[first + i];
      g.x[i] = q.x;
      g.q[i] = q.q;
      g.s[i] = q.s;
      g.qt[i] = q.qt;
      g.st[i] = q.st;
      g.ld[i] = q.ld;
      g.rows[i] = (int)q.rows;
      g.cols[i] = (int)q.cols;
      g.block_base[i] = (int)base;
      // row tiles: the transposed copy is written over its whole padded width roundup(rows, 128)
      const int64_t row_tiles = q.qt ? (q.rows + 127) / 128 * 4 : (q.rows + 31) / 32;
      base += row_tiles * ((q.cols + 127) / 128);
      PLM_REQUIRE(base < (1ll << 31), "plm_mx_quant_multi: too many tiles");
    }
    g.block_base[n] = (int)base;
    g.count = n;
    hipLaunchKernelGGL(mx_quant_kernel, dim3((unsigned)base), dim3(128), 0, (hipStream_t)stream, g);
    PLM_CHECK_LAUNCH("plm_mx_quant_multi");
  }
  return PLM_OK;
}

extern "C" int plm_mx_quant(const uint16_t* x, int64_t ld, int64_t rows, int64_t cols, uint8_t* q, uint8_t* s, uint8_t* qt, uint8_t* st,
                            void* stream) {
  const plm_mx_quant_item it{x, ld, rows, cols, q, s, qt, st};
  const int rc = mx_check_item(it, "plm_mx_quant", 0);
  return rc != PLM_OK ? rc : plm_mx_quant_multi(&it, 1, stream);
}

// ---------------------------------------------------------------------------
// MX NT GEMM
// ---------------------------------------------------------------------------
// 128 x 128 output tile, 256 threads = 4 waves as 2 (M) x 2 (N), wave tile 64 x 64 = 2 x 2 accumulators of
// v_mfma_scale_f32_32x32x64_f8f6f4.  K-step BK = 128 elements: one 128-byte line per operand row and one scale dword per row (the
// 4 blocks of the step).  Three LDS stages, all in one __shared__ array, filled only by LDS-DMA (data 16 B per lane, scales 4 B per
// lane: one load kind, so hipcc's own waits never drain the ring); one K-step = counted s_waitcnt vmcnt (the next tile stays in
// flight), one barrier, the DMA of tile t + 2, 8 MFMAs per wave.
//
// Operand lane maps (measured on the MI355X with exact small-integer data and per-block scales; pinned by tests/test_mx_gpu.py): lane l
// holds row l & 31 of A (column l & 31 of B^T); with h = l >> 5, bytes 0..15 of its 8 dwords are k = 16h + j and bytes 16..31 are
// k = 32 + 16h + (j - 16).  The 32-element block 0 (k 0..31) is thus spread over both lane halves, and takes its E8M0 scale from the
// lanes with h = 0, block 1 (k 32..63) from h = 1 (scale in byte 0 of the scale VGPR, op_sel 0).  C/D: col = l & 31,
// row = mfma32_row(reg, h), as for bf16.
constexpr int MX_BM = 128, MX_BN = 128;
constexpr int MX_TILE = 128 * 128;             // bytes of one operand's K-step
constexpr int MX_STAGE = 2 * MX_TILE + 1024;   // A, B, then 128 A-scale and 128 B-scale dwords
constexpr int MX_NSTAGE = 3;
constexpr int MX_LOADS = 9;                    // DMA instructions per thread per K-step: 4 (A) + 4 (B) + 1 (scales)

__device__ __forceinline__ void dma4_asm(const void* gsrc, unsigned lds_wave_addr) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_wave_addr);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(dst)
               : "memory");
}
__device__ __forceinline__ void dma16_u32(const void* gsrc, unsigned lds_wave_addr) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_wave_addr);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(dst)
               : "memory");
}
// vmcnt(last ? 0 : MX_LOADS): the branch keeps the drain out of the steady-state K-loop
__device__ __forceinline__ void mx_wait(int last) {
  asm volatile("s_cmp_lg_u32 %0, 0\n\ts_cbranch_scc1 1f\n\ts_waitcnt vmcnt(%1)\n\ts_branch 2f\n1:\n\ts_waitcnt vmcnt(0)\n2:" ::"s"(last), "n"(MX_LOADS)
               : "memory", "scc");
}
__device__ __forceinline__ void mx_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// LDS image of an operand K-step: [128 rows][128 B], 16-byte chunk c of row r at chunk position c ^ (r & 7) (conflict-free b128 reads)
__device__ __forceinline__ int mx_swz(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }

__global__ __launch_bounds__(256, 1) void gemm_mx_nt_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ As,
                                                            const uint8_t* __restrict__ B, const uint8_t* __restrict__ Bs, void* __restrict__ C,
                                                            int64_t ldc, int M, int N, int Kp, int mode, int tiles_n) {
  __shared__ __attribute__((aligned(1024))) char smem[MX_NSTAGE * MX_STAGE];
  const int nwg = gridDim.x;
  const int bid = xcd_remap(blockIdx.x, nwg);
  const int m0 = (bid / tiles_n) * MX_BM, n0 = (bid % tiles_n) * MX_BN;
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int wr = w >> 1, wc = w & 1, h = l >> 5, l31 = l & 31;
  const int64_t ks = Kp >> 5;  // scale bytes per row
  const int nk = Kp >> 7;
  const unsigned lds0 = lds_addr_u32(smem);

  // per-thread DMA sources: operand rows (clamped to the last row: the tail tile's extra rows are never stored)
  const uint8_t* srcA[4];
  const uint8_t* srcB[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int g8 = i * 4 + w, row = 8 * g8 + (l >> 3), chunk = (l & 7) ^ (row & 7);
    srcA[i] = A + (int64_t)min(m0 + row, M - 1) * Kp + (chunk << 4);
    srcB[i] = B + (int64_t)min(n0 + row, N - 1) * Kp + (chunk << 4);
  }
  const uint8_t* srcS = w < 2 ? As + (int64_t)min(m0 + 64 * w + l, M - 1) * ks : Bs + (int64_t)min(n0 + 64 * (w - 2) + l, N - 1) * ks;
  auto issue = [&](int kt, int stage) {
    const unsigned base = lds0 + stage * MX_STAGE;
    const int64_t kb = (int64_t)kt * 128;
#pragma unroll
    for (int i = 0; i < 4; ++i) dma16_u32(srcA[i] + kb, base + (i * 4 + w) * 1024);
#pragma unroll
    for (int i = 0; i < 4; ++i) dma16_u32(srcB[i] + kb, base + MX_TILE + (i * 4 + w) * 1024);
    dma4_asm(srcS + kt * 4, base + 2 * MX_TILE + w * 256);
  };

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  issue(0, 0);
  if (nk > 1) issue(1, 1);
  int stage = 0;
  for (int kt = 0; kt < nk; ++kt) {
    mx_wait(__builtin_amdgcn_readfirstlane(kt + 1 >= nk ? 1 : 0));
    mx_barrier();
    if (kt + 2 < nk) issue(kt + 2, stage == 0 ? 2 : stage - 1);
    const char* sa = smem + stage * MX_STAGE;
    const char* sb = sa + MX_TILE;
    const unsigned* ssa = reinterpret_cast<const unsigned*>(sa + 2 * MX_TILE);
    const unsigned* ssb = ssa + 128;
    i32x8_t fa[2][2], fb[2][2];
    unsigned sca[2], scb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int ra = wr * 64 + i * 32 + l31, rb = wc * 64 + i * 32 + l31;
      sca[i] = ssa[ra];
      scb[i] = ssb[rb];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int c = 4 * s + h;  // k 16h ...+15 and 32 + 16h ...+15 of the sub-step (the operand map above)
        const u32x4_t a0 = *reinterpret_cast<const u32x4_t*>(sa + mx_swz(ra, c));
        const u32x4_t a1 = *reinterpret_cast<const u32x4_t*>(sa + mx_swz(ra, c + 2));
        const u32x4_t b0 = *reinterpret_cast<const u32x4_t*>(sb + mx_swz(rb, c));
        const u32x4_t b1 = *reinterpret_cast<const u32x4_t*>(sb + mx_swz(rb, c + 2));
        fa[i][s] = i32x8_t{(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
        fb[i][s] = i32x8_t{(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3], (int)b1[0], (int)b1[1], (int)b1[2], (int)b1[3]};
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int sh = 8 * (2 * s + h);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0, (int)((sca[i] >> sh) & 0xFFu), 0,
                                                                      (int)((scb[j] >> sh) & 0xFFu));
    }
    stage = stage == 2 ? 0 : stage + 1;
  }

  // epilogue: each element is owned by one lane (no atomics); lanes 0..31 of a register cover 32 consecutive columns
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wc * 64 + j * 32 + l31;
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wr * 64 + i * 32 + mfma32_row(r, h);
        if (row >= M) continue;
        const int64_t off = (int64_t)row * ldc + col;
        if (mode == PLM_MX_OUT_BF16) {
          reinterpret_cast<bf16_t*>(C)[off] = f2bf(acc[i][j][r]);
        } else if (mode == PLM_MX_OUT_F32) {
          reinterpret_cast<float*>(C)[off] = acc[i][j][r];
        } else {
          reinterpret_cast<float*>(C)[off] += acc[i][j][r];
        }
      }
    }
}

extern "C" int plm_gemm_mx_nt(const uint8_t* A, const uint8_t* As, const uint8_t* B, const uint8_t* Bs, void* C, int64_t ldc, int64_t M, int64_t N,
                              int64_t Kp, int mode, void* stream) {
  PLM_REQUIRE(A && As && B && Bs && C, "plm_gemm_mx_nt: null pointer");
  PLM_REQUIRE(M > 0 && N > 0 && M < (1ll << 30) && N < (1ll << 30), "plm_gemm_mx_nt: M=%ld N=%ld must be positive", (long)M, (long)N);
  PLM_REQUIRE(Kp > 0 && Kp % 128 == 0 && Kp < (1ll << 30), "plm_gemm_mx_nt: Kp=%ld must be a positive multiple of 128", (long)Kp);
  PLM_REQUIRE(ldc >= N, "plm_gemm_mx_nt: ldc=%ld < N=%ld", (long)ldc, (long)N);
  PLM_REQUIRE(mode == PLM_MX_OUT_BF16 || mode == PLM_MX_OUT_F32 || mode == PLM_MX_OUT_F32_ACC, "plm_gemm_mx_nt: unknown output mode %d", mode);
  PLM_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)B & 15) == 0 && ((uintptr_t)As & 3) == 0 && ((uintptr_t)Bs & 3) == 0 &&
                  ((uintptr_t)C & (mode == PLM_MX_OUT_BF16 ? 1 : 3)) == 0,
              "plm_gemm_mx_nt: A and B must be 16-byte aligned, the scales 4-byte aligned, C aligned to its element");
  const int64_t tiles_m = plm_cdiv(M, MX_BM), tiles_n = plm_cdiv(N, MX_BN);
  PLM_REQUIRE(tiles_m * tiles_n < (1ll << 31), "plm_gemm_mx_nt: too many tiles");
  hipLaunchKernelGGL(gemm_mx_nt_kernel, dim3((unsigned)(tiles_m * tiles_n)), dim3(256), 0, (hipStream_t)stream, A, As, B, Bs, C, ldc, (int)M, (int)N,
                     (int)Kp, mode, (int)tiles_n);
  PLM_CHECK_LAUNCH("plm_gemm_mx_nt");
  return PLM_OK;
}
