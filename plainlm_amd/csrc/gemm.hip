// bf16 MFMA GEMMs for gfx950 (v_mfma_f32_32x32x16_bf16, fp32 accumulate).
//
//   nt : C[M,N] = alpha * A[M,K] · B[N,K]^T      (y = x W^T ; dX = dY (W^T)^T with the transposed weight copy)
//   tn : C[M,N] (+)= alpha * A[K,M]^T · B[K,N]    (dW = dY^T X, contraction over the token rows)
//
// Structure (both): 128x128 output tile per 256-thread workgroup (4 waves as 2x2, each wave a 64x64
// sub-tile = 2x2 MFMA 32x32 accumulators), BK = 64, operands staged global -> registers -> LDS with the
// next tile's global loads in flight during the MFMAs of the current one (one LDS buffer, two barriers
// per K-step, ~3 workgroups per CU so other workgroups cover the barrier bubbles).
//
// nt LDS image: [128 rows][64 k] bf16 (128-byte rows); the 16-byte chunk index is XOR-ed with
//   (row>>1)&7 so the sixteen lanes of a ds_read_b128 service group (16 distinct rows mod 16, same
//   k-chunk) hit sixteen different 16-byte slots of the 256-byte bank row: conflict-free.
// tn LDS image: [8 column-subtiles][64 k-rows][16 cols] (32-byte rows, sub-tile stride 2048+128 B) read
//   with ds_read_b64_tr_b16, which hands lane t column t of a [4 k][16 col] block: the MFMA operand
//   with k = token row.  A 32-lane half covers two sub-tiles 128 B apart mod 256: conflict-free.
//
// Workgroup -> tile map: XCD-aware remap (each XCD gets a contiguous id range) and grouped
// rasterisation (GROUP_M row-panels x all column tiles) so A panels and B tiles are reused from L2.
#include <stdlib.h>

#include "gemm_launch.h"

#define GBM 128
#define GBN 128
#define GBK 64
#define GROUP_M 8
#define TN_SUB_STRIDE 2176  // 64 rows * 32 B + 128 B pad

__device__ __forceinline__ void tile_coords(int bid, int nwg, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int pid = xcd_remap(bid, nwg);
  const int group_size = GROUP_M * tiles_n;
  const int group = pid / group_size;
  const int first_m = group * GROUP_M;
  const int gm = min(tiles_m - first_m, GROUP_M);
  const int in_group = pid - group * group_size;
  tm = first_m + in_group % gm;
  tn = in_group / gm;
}

// ---------------------------------------------------------------------------------------------
// NT
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int nt_lds_off(int row, int chunk) {  // byte offset of a 16-byte chunk
  return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

template <bool OUT_F32, bool ACCUM>
__global__ __launch_bounds__(256) void gemm_nt_kernel(const uint16_t* __restrict__ A, int64_t lda,
                                                      const uint16_t* __restrict__ B, int64_t ldb, void* __restrict__ Cv,
                                                      int64_t ldc, int M, int N, int K, const float* __restrict__ alpha_dev,
                                                      int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) char smem[2 * GBM * GBK * 2];
  char* sA = smem;
  char* sB = smem + GBM * GBK * 2;

  int tm, tn;
  tile_coords(blockIdx.x, gridDim.x, tiles_m, tiles_n, tm, tn);
  const int m0 = tm * GBM, n0 = tn * GBN;
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
      const bool kin = (k0 + ld_chunk[i] * 8) < K;
      ra[i] = (a_ok[i] && kin) ? ld_bf16x8(a_ptr[i] + k0) : zero_bf16x8();
      rb[i] = (b_ok[i] && kin) ? ld_bf16x8(b_ptr[i] + k0) : zero_bf16x8();
    }
  };
  auto s_store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = nt_lds_off(ld_row[i], ld_chunk[i]);
      *reinterpret_cast<bf16x8_t*>(sA + off) = ra[i];
      *reinterpret_cast<bf16x8_t*>(sB + off) = rb[i];
    }
  };

  const int nk = (K + GBK - 1) / GBK;
  g_load(0);
  s_store();
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) g_load((kt + 1) * GBK);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8_t af[2], bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = *reinterpret_cast<const bf16x8_t*>(sA + nt_lds_off(wm * 64 + i * 32 + l31, ks * 2 + hi));
        bfr[i] = *reinterpret_cast<const bf16x8_t*>(sB + nt_lds_off(wn * 64 + i * 32 + l31, ks * 2 + hi));
      }
      // D'[n][m] = sum_k B[n][k] A[m][k]: the lane ends up owning one C row (m) and runs of 4 consecutive n
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(bfr[j], af[i], acc[i][j]);
    }
    __syncthreads();
    if (kt + 1 < nk) {
      s_store();
      __syncthreads();
    }
  }

  const float alpha = alpha_dev ? *alpha_dev : 1.f;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + wm * 64 + i * 32 + l31;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * 64 + j * 32 + 8 * g + 4 * hi;
        if (n >= N) continue;
        f32x4_t v = {acc[i][j][4 * g + 0] * alpha, acc[i][j][4 * g + 1] * alpha, acc[i][j][4 * g + 2] * alpha,
                     acc[i][j][4 * g + 3] * alpha};
        if (OUT_F32) {
          float* dst = reinterpret_cast<float*>(Cv) + (int64_t)m * ldc + n;
          if (n + 3 < N) {
            if (ACCUM) v += *reinterpret_cast<const f32x4_t*>(dst);
            *reinterpret_cast<f32x4_t*>(dst) = v;
          } else {
            for (int e = 0; e < 4 && n + e < N; ++e) dst[e] = ACCUM ? dst[e] + v[e] : v[e];
          }
        } else {
          uint16_t* dst = reinterpret_cast<uint16_t*>(Cv) + (int64_t)m * ldc + n;
          bf16x4_t o;
          o[0] = f2bf(v[0]); o[1] = f2bf(v[1]); o[2] = f2bf(v[2]); o[3] = f2bf(v[3]);
          if (n + 3 < N) {
            st_bf16x4(dst, o);
          } else {
            for (int e = 0; e < 4 && n + e < N; ++e) reinterpret_cast<bf16_t*>(dst)[e] = o[e];
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// NT v2: operands go global -> LDS by LDS-DMA (global_load_lds_dwordx4: no VGPR round trip, no ds_write),
// two LDS buffers, ONE barrier per K-step; C leaves through LDS as full 128-byte row segments.
// The DMA writes lane-linear (wave-uniform base + lane*16 B), so the XOR swizzle of nt_lds_off() is applied
// to the per-lane SOURCE address: LDS slot s of row r receives global chunk s ^ ((r>>1)&7).
// Needs K % 64 == 0 (no K tail), N % 8 == 0 and 16-byte aligned C rows; other shapes use gemm_nt_kernel.
// ---------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void gbl_void_t;

__device__ __forceinline__ void dma16(const void* gsrc, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((gbl_void_t*)gsrc, (lds_void_t*)lds_wave_base, 16, 0, 0);
}

#define EPI_STRIDE_BF16 144   // 64 bf16 + 16 B pad: 16-byte aligned rows, 2-way at worst on the 8-byte writes
#define EPI_STRIDE_F32 272    // 64 fp32 + 16 B pad

template <bool OUT_F32, bool ACCUM>
__global__ __launch_bounds__(256) void gemm_nt_dma_kernel(const uint16_t* __restrict__ A, int64_t lda,
                                                          const uint16_t* __restrict__ B, int64_t ldb, void* __restrict__ Cv,
                                                          int64_t ldc, int M, int N, int K, const float* __restrict__ alpha_dev,
                                                          int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * 2 * GBM * GBK * 2];  // [buf][A|B][16 KiB]
  int tm, tn;
  tile_coords(blockIdx.x, gridDim.x, tiles_m, tiles_n, tm, tn);
  const int m0 = tm * GBM, n0 = tn * GBN;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, hi = lane >> 5;

  // DMA assignment: instruction i of wave w fills LDS rows (i*4+w)*8 .. +7 (1 KiB); lane -> (row, slot)
  const uint16_t* a_src[4];
  const uint16_t* b_src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (i * 4 + wave) * 8 + (lane >> 3);
    const int chunk = (lane & 7) ^ ((row >> 1) & 7);
    const int ar = min(m0 + row, M - 1), br = min(n0 + row, N - 1);  // tail rows: any valid address, results unused
    a_src[i] = A + (int64_t)ar * lda + chunk * 8;
    b_src[i] = B + (int64_t)br * ldb + chunk * 8;
  }
  auto dma_tile = [&](int buf, int k0) {
    char* dA = smem + buf * (2 * GBM * GBK * 2);
    char* dB = dA + GBM * GBK * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      dma16(a_src[i] + k0, dA + (i * 4 + wave) * 1024);
      dma16(b_src[i] + k0, dB + (i * 4 + wave) * 1024);
    }
  };

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = K / GBK;
  dma_tile(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) dma_tile(cur ^ 1, (kt + 1) * GBK);
    const char* sA = smem + cur * (2 * GBM * GBK * 2);
    const char* sB = sA + GBM * GBK * 2;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8_t af[2], bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = *reinterpret_cast<const bf16x8_t*>(sA + nt_lds_off(wm * 64 + i * 32 + l31, ks * 2 + hi));
        bfr[i] = *reinterpret_cast<const bf16x8_t*>(sB + nt_lds_off(wn * 64 + i * 32 + l31, ks * 2 + hi));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(bfr[j], af[i], acc[i][j]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA pieces of the next tile have landed
    __syncthreads();                                   // ... and everyone's; also: all reads of buf[cur] are done
  }

  // ---- epilogue: accumulators -> LDS (per-wave region) -> 16-byte row-contiguous global stores ----
  const float alpha = alpha_dev ? *alpha_dev : 1.f;
  constexpr int STRIDE = OUT_F32 ? EPI_STRIDE_F32 : EPI_STRIDE_BF16;
  char* epi = smem + wave * (32 * STRIDE);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    // 32 rows (m) x 64 cols (n) of this wave: lane owns row l31, 4-column runs
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = j * 32 + 8 * g + 4 * hi;
        f32x4_t v = {acc[i][j][4 * g + 0] * alpha, acc[i][j][4 * g + 1] * alpha, acc[i][j][4 * g + 2] * alpha,
                     acc[i][j][4 * g + 3] * alpha};
        if (OUT_F32) {
          *reinterpret_cast<f32x4_t*>(epi + l31 * STRIDE + col * 4) = v;
        } else {
          bf16x4_t o;
          o[0] = f2bf(v[0]); o[1] = f2bf(v[1]); o[2] = f2bf(v[2]); o[3] = f2bf(v[3]);
          *reinterpret_cast<bf16x4_t*>(epi + l31 * STRIDE + col * 2) = o;
        }
      }
    }
    __syncthreads();
    constexpr int CPR = OUT_F32 ? 16 : 8;            // 16-byte chunks per 64-column row
    constexpr int ITERS = 32 * CPR / 64;             // per-lane chunks for 32 rows
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int c = it * 64 + lane;
      const int row = c / CPR, cc = c % CPR;
      const int gm = m0 + wm * 64 + i * 32 + row;
      const int gn = n0 + wn * 64 + cc * (OUT_F32 ? 4 : 8);
      if (gm < M && gn < N) {
        if (OUT_F32) {
          f32x4_t v = *reinterpret_cast<const f32x4_t*>(epi + row * STRIDE + cc * 16);
          float* dst = reinterpret_cast<float*>(Cv) + (int64_t)gm * ldc + gn;
          if (ACCUM) v += *reinterpret_cast<const f32x4_t*>(dst);
          *reinterpret_cast<f32x4_t*>(dst) = v;
        } else {
          const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(epi + row * STRIDE + cc * 16);
          st_bf16x8(reinterpret_cast<uint16_t*>(Cv) + (int64_t)gm * ldc + gn, v);
        }
      }
    }
    if (i == 0) __syncthreads();
  }
}

void plm_launch_gemm_nt_128(const NtPlan& p, const GemmOperands& o, int c_dtype, int accumulate, hipStream_t s) {
  const dim3 grid((unsigned)p.grid), block(256);
#define PLM_NT_LAUNCH(KERN)                                                                                                    \
  hipLaunchKernelGGL(KERN, grid, block, 0, s, o.A, o.lda, o.B, o.ldb, o.C, o.ldc, (int)o.M, (int)o.N, (int)o.K, o.alpha_dev, p.tm, p.tn)
  if (p.kernel == NT_DMA128) {
    if (c_dtype == 0) PLM_NT_LAUNCH((gemm_nt_dma_kernel<false, false>));
    else if (accumulate) PLM_NT_LAUNCH((gemm_nt_dma_kernel<true, true>));
    else PLM_NT_LAUNCH((gemm_nt_dma_kernel<true, false>));
  } else {
    if (c_dtype == 0) PLM_NT_LAUNCH((gemm_nt_kernel<false, false>));
    else if (accumulate) PLM_NT_LAUNCH((gemm_nt_kernel<true, true>));
    else PLM_NT_LAUNCH((gemm_nt_kernel<true, false>));
  }
#undef PLM_NT_LAUNCH
}

// ---------------------------------------------------------------------------------------------
// TN   C[i][j] = sum_k A[k][i] B[k][j]
// ---------------------------------------------------------------------------------------------
// MODE 0: C = alpha*acc   MODE 1: C += alpha*acc   MODE 2: raw partial into a split-K slab (ld = N)
template <int MODE>
__global__ __launch_bounds__(256) void gemm_tn_kernel(const uint16_t* __restrict__ A, int64_t lda,
                                                      const uint16_t* __restrict__ B, int64_t ldb, float* __restrict__ C,
                                                      int64_t ldc, int M, int N, int K, int kchunk,
                                                      const float* __restrict__ alpha_dev, int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 8 * TN_SUB_STRIDE];
  char* sA = smem;
  char* sB = smem + 8 * TN_SUB_STRIDE;

  int tm, tn;
  tile_coords(blockIdx.x, gridDim.x, tiles_m, tiles_n, tm, tn);
  const int i0 = tm * GBM, j0 = tn * GBN;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(K, kbeg + kchunk);
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, hi = lane >> 5, ib = (lane >> 4) & 1, t16 = lane & 15;

  int ld_krow[4], ld_off[4];
  const uint16_t* a_ptr[4];
  const uint16_t* b_ptr[4];
  bool a_ok[4], b_ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = i * 256 + t;
    const int u = idx & 7, cl = u & 3, rl = u >> 2, rest = idx >> 3;
    const int c = (rest & 3) * 4 + cl;           // 16-byte chunk along the 128 columns
    ld_krow[i] = ((rest >> 2) << 1) | rl;        // 0..63
    ld_off[i] = (c >> 1) * TN_SUB_STRIDE + ld_krow[i] * 32 + (c & 1) * 16;
    a_ok[i] = (i0 + c * 8) < M;
    b_ok[i] = (j0 + c * 8) < N;
    a_ptr[i] = A + (int64_t)ld_krow[i] * lda + i0 + c * 8;
    b_ptr[i] = B + (int64_t)ld_krow[i] * ldb + j0 + c * 8;
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
      const bool kin = (k0 + ld_krow[i]) < kend;
      ra[i] = (a_ok[i] && kin) ? ld_bf16x8(a_ptr[i] + (int64_t)k0 * lda) : zero_bf16x8();
      rb[i] = (b_ok[i] && kin) ? ld_bf16x8(b_ptr[i] + (int64_t)k0 * ldb) : zero_bf16x8();
    }
  };
  auto s_store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<bf16x8_t*>(sA + ld_off[i]) = ra[i];
      *reinterpret_cast<bf16x8_t*>(sB + ld_off[i]) = rb[i];
    }
  };
  // transpose-read of one 32-column operand block starting at tile column cb, k-step ks
  auto tr_frag = [&](const char* base, int cb, int ks) -> bf16x8_t {
    const char* p = base + ((cb >> 4) + ib) * TN_SUB_STRIDE + (ks * 16 + hi * 8 + (t16 >> 2)) * 32 + (t16 & 3) * 8;
    const s16x4_t lo = lds_read_tr16(p);
    const s16x4_t hh = lds_read_tr16(p + 4 * 32);
    return join_tr(lo, hh);
  };

  const int nk = (kend - kbeg + GBK - 1) / GBK;
  if (nk > 0) {
    g_load(kbeg);
    s_store();
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) g_load(kbeg + (kt + 1) * GBK);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8_t af[2], bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = tr_frag(sA, wm * 64 + i * 32, ks);
        bfr[i] = tr_frag(sB, wn * 64 + i * 32, ks);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(af[i], bfr[j], acc[i][j]);
    }
    __syncthreads();
    if (kt + 1 < nk) {
      s_store();
      __syncthreads();
    }
  }

  const float alpha = (MODE != 2 && alpha_dev) ? *alpha_dev : 1.f;
  float* out = (MODE == 2) ? C + (int64_t)blockIdx.y * M * N : C;
  const int64_t ld = (MODE == 2) ? N : ldc;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = j0 + wn * 64 + j * 32 + l31;
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = i0 + wm * 64 + i * 32 + mfma32_row(r, hi);
        if (row >= M) continue;
        float* dst = out + (int64_t)row * ld + col;
        const float v = acc[i][j][r] * alpha;
        *dst = (MODE == 1) ? *dst + v : v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// TN v2: LDS-DMA + two LDS buffers + one barrier per K-step (needs K and the split chunk % 64 == 0).
// LDS image per operand: [64 k-rows][128 cols] bf16, 256-byte rows, written lane-linear by the DMA
// (one wave-instruction = 4 full rows: perfectly coalesced source reads).  The 32-byte column pairs of
// row k are ROTATED by 2*(k&3) pair positions (on the source address): the four rows of a transpose-read
// block then sit on four different 32-byte bank segments and the two 16-lane groups of a half-wave use
// the even/odd segments: ds_read_b64_tr_b16 is conflict-free.
// ---------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void gemm_tn_dma_kernel(const uint16_t* __restrict__ A, int64_t lda,
                                                          const uint16_t* __restrict__ B, int64_t ldb, float* __restrict__ C,
                                                          int64_t ldc, int M, int N, int K, int kchunk,
                                                          const float* __restrict__ alpha_dev, int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * 2 * GBK * GBM * 2];  // [buf][A|B][16 KiB]
  int tm, tn;
  tile_coords(blockIdx.x, gridDim.x, tiles_m, tiles_n, tm, tn);
  const int i0 = tm * GBM, j0 = tn * GBN;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = min(K, kbeg + kchunk);
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, hi = lane >> 5, ib = (lane >> 4) & 1, t16 = lane & 15;

  const uint16_t* a_src[4];
  const uint16_t* b_src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (i * 4 + wave) * 4 + (lane >> 4);      // k-row inside the tile
    const int pp = (lane & 15) >> 1, half = lane & 1;       // physical 32-byte pair / 16-byte half
    const int cb = (pp - 2 * (row & 3)) & 7;                // logical pair stored there
    const int col = cb * 16 + half * 8;
    a_src[i] = A + (int64_t)row * lda + min(i0 + col, M - 8);  // column tails: any valid address, results unused
    b_src[i] = B + (int64_t)row * ldb + min(j0 + col, N - 8);
  }
  auto dma_tile = [&](int buf, int k0) {
    char* dA = smem + buf * (2 * GBK * GBM * 2);
    char* dB = dA + GBK * GBM * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      dma16_asm(a_src[i] + (int64_t)k0 * lda, dA + (i * 4 + wave) * 1024);
      dma16_asm(b_src[i] + (int64_t)k0 * ldb, dB + (i * 4 + wave) * 1024);
    }
  };
  auto tr_frag = [&](const char* base, int cb0, int ks) -> bf16x8_t {
    const int row = ks * 16 + hi * 8 + (t16 >> 2);
    const char* p = base + row * 256 + (((cb0 + ib) + 2 * (row & 3)) & 7) * 32 + (t16 & 3) * 8;
    return join_tr(lds_read_tr16(p), lds_read_tr16(p + 4 * 256));
  };

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = (kend - kbeg) / GBK;
  if (nk > 0) dma_tile(0, kbeg);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) dma_tile(cur ^ 1, kbeg + (kt + 1) * GBK);
    const char* sA = smem + cur * (2 * GBK * GBM * 2);
    const char* sB = sA + GBK * GBM * 2;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8_t af[2], bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = tr_frag(sA, (wm * 64 + i * 32) >> 4, ks);
        bfr[i] = tr_frag(sB, (wn * 64 + i * 32) >> 4, ks);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma32(af[i], bfr[j], acc[i][j]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  const float alpha = (MODE != 2 && alpha_dev) ? *alpha_dev : 1.f;
  float* out = (MODE == 2) ? C + (int64_t)blockIdx.y * M * N : C;
  const int64_t ld = (MODE == 2) ? N : ldc;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = j0 + wn * 64 + j * 32 + l31;
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = i0 + wm * 64 + i * 32 + mfma32_row(r, hi);
        if (row >= M) continue;
        float* dst = out + (int64_t)row * ld + col;
        const float v = acc[i][j][r] * alpha;
        *dst = (MODE == 1) ? *dst + v : v;
      }
    }
  }
}

// C (+)= alpha * sum_s slab[s]
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, float* __restrict__ C, int64_t ldc, int M,
                                                            int N, int splits, int accumulate,
                                                            const float* __restrict__ alpha_dev) {
  const float alpha = alpha_dev ? *alpha_dev : 1.f;
  const int64_t nv = (int64_t)M * (N >> 2);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int nq = N >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    const int64_t row = i / nq;
    const int col = (int)(i - row * nq) * 4;
    f32x4_t s = *reinterpret_cast<const f32x4_t*>(ws + row * N + col);
    for (int k = 1; k < splits; ++k) s += *reinterpret_cast<const f32x4_t*>(ws + (int64_t)k * M * N + row * N + col);
    s *= alpha;
    float* dst = C + row * ldc + col;
    if (accumulate) s += *reinterpret_cast<const f32x4_t*>(dst);
    *reinterpret_cast<f32x4_t*>(dst) = s;
  }
}

// splits == 1: C (+)= alpha*acc directly (MODE 0 / 1); otherwise raw partials into the slabs (MODE 2), summed by plm_launch_splitk_reduce
void plm_launch_gemm_tn_128(const TnPlan& p, const GemmOperands& o, int accumulate, float* slabs, hipStream_t s) {
  const dim3 grid((unsigned)p.grid, (unsigned)p.splits), block(256);
#define PLM_TN_LAUNCH(KERN, C_, LDC_, ALPHA_)                                                                                      \
  hipLaunchKernelGGL(KERN, grid, block, 0, s, o.A, o.lda, o.B, o.ldb, C_, LDC_, (int)o.M, (int)o.N, (int)o.K, p.kchunk, ALPHA_, p.tm, p.tn)
  if (p.kernel == TN_DMA128) {
    if (p.splits > 1) PLM_TN_LAUNCH(gemm_tn_dma_kernel<2>, slabs, o.N, (const float*)nullptr);
    else if (accumulate) PLM_TN_LAUNCH(gemm_tn_dma_kernel<1>, (float*)o.C, o.ldc, o.alpha_dev);
    else PLM_TN_LAUNCH(gemm_tn_dma_kernel<0>, (float*)o.C, o.ldc, o.alpha_dev);
  } else {
    if (p.splits > 1) PLM_TN_LAUNCH(gemm_tn_kernel<2>, slabs, o.N, (const float*)nullptr);
    else if (accumulate) PLM_TN_LAUNCH(gemm_tn_kernel<1>, (float*)o.C, o.ldc, o.alpha_dev);
    else PLM_TN_LAUNCH(gemm_tn_kernel<0>, (float*)o.C, o.ldc, o.alpha_dev);
  }
#undef PLM_TN_LAUNCH
}

void plm_launch_splitk_reduce(const TnPlan& p, const GemmOperands& o, int accumulate, float* slabs, hipStream_t s) {
  const int64_t nv = p.split_rows * (o.N / 4);
  int64_t rb = plm_cdiv(nv, 256);
  if (rb > 4096) rb = 4096;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, s, (const float*)slabs, (float*)o.C + (int64_t)p.rfull * 256 * o.ldc, o.ldc,
                     (int)p.split_rows, (int)o.N, p.splits, accumulate, o.alpha_dev);
}
