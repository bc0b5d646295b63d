// Launch plans of the bf16 GEMMs: which kernel, which tile, which grid, how much workspace.  Arithmetic on shapes only - plain C++17,
// no HIP - so every function takes the shape, `slots` (persistent workgroups: CUs minus the reserve) and the environment switches as
// values.  The entry points (gemm_api.hip) make ONE plan per call and hand it to the workspace query and to the launch alike.
#pragma once

#include <stddef.h>
#include <stdint.h>

static inline int64_t plan_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the PlmEnv switches the plans depend on
struct GemmPlanEnv {
  bool gemm_v1, tn_no_big, nt_no_hybrid;
  long long nt_hybrid_min_k;
};

static inline double round_efficiency(int64_t tiles, int slots) {
  const int64_t rounds = (tiles + slots - 1) / slots;
  return (double)tiles / (double)(rounds * slots);
}

// ---------------------------------------------------------------------------------------------
// NT
// ---------------------------------------------------------------------------------------------
// Tile shapes of the persistent NT kernel and the automatic policy that picks one per launch: round efficiency of the tile count on the
// persistent grid x the useful fraction of the (ragged) edge tiles x a measured per-tile rate relative to 256x256.  256x192 has 22 % fewer
// LDS-DMA bytes and 17 % fewer LDS reads per MFMA than 256x128, and N = 768 is four 192-column tiles = exactly two rounds at M = 32768;
// 256x256 at 0.90 round efficiency beats 256x128 at 1.0 on the qkv shape.  128x192 (round 5; 8 waves of 32x96) is the shape of the
// short batches: M = 8192 (the reference's document-mask config, config_doc_mask.yaml:35) makes N = 768 exactly ONE round of 256 tiles
// and N = 2304 exactly three, where every 256-row tile leaves 25-62 % of the chip idle.
// Rates fitted on the kbench --variants tables at M = 8192 / 16384 / 32768 (profiles/r05_kbench_variants.txt).
// Order = preference on ties (the first strictly greater wins).
struct NtTileShape {
  int bm, bn;
  double rate;
};
static const NtTileShape kNtTiles[4] = {{256, 256, 1.0}, {256, 128, 0.88}, {256, 192, 0.94}, {128, 192, 0.72}};
static const int kNtTileVariant[4] = {4, 6, 5, 7};  // the explicit variant number of each (plm_gemm_bf16_nt_ex)
static inline double nt_tile_eff(int i, int64_t M, int64_t N, int slots) {
  const NtTileShape& t = kNtTiles[i];
  const int64_t tm = plan_cdiv(M, t.bm), tn = plan_cdiv(N, t.bn);
  return round_efficiency(tm * tn, slots) * ((double)N / (double)(tn * t.bn)) * ((double)M / (double)(tm * t.bm)) * t.rate;
}
// index into kNtTiles of the best shape, its efficiency in *eff
static inline int nt_pick_tile(int64_t M, int64_t N, int slots, double* eff) {
  int best = 0;
  double be = -1.0;
  for (int i = 0; i < 4; ++i) {
    const double e = nt_tile_eff(i, M, N, slots);
    if (e > be) {
      be = e;
      best = i;
    }
  }
  *eff = be;
  return best;
}
// the hardware-scheduled 128x128 LDS-DMA kernel of gemm.hip (two 4-wave workgroups per CU, ~0.8 of the persistent 256x256 per-tile rate)
// on the same scale: what the persistent kernels have to beat
static inline double nt_dma128_eff(int64_t M, int64_t N, int slots) {
  const int64_t tm = plan_cdiv(M, 128), tn = plan_cdiv(N, 128);
  return round_efficiency(tm * tn, 2 * slots) * ((double)N / (double)(tn * 128)) * ((double)M / (double)(tm * 128)) * 0.80;
}

// what the LDS-DMA kernels (128x128 and persistent) need of a shape: no K tail, 16-byte row segments of C
static inline bool nt_dma_shape(int64_t N, int64_t K, int64_t ldc) { return (K % 64 == 0) && (N % 8 == 0) && (ldc % 8 == 0); }

enum NtEpilogue { NT_EPI_NONE, NT_EPI_ROPE, NT_EPI_GLU, NT_EPI_GLUB, NT_EPI_SCORE };
enum NtKernel {
  NT_REG128,      // gemm_nt_kernel: register-staged 128x128, any shape
  NT_DMA128,      // gemm_nt_dma_kernel: LDS-DMA 128x128
  NT_PERSISTENT,  // gemm_nt_big_kernel on tile kNtTiles[tile], plain schedule
  NT_HYBRID       // gemm_nt_big_kernel<256, 256, HYB> + nt_streamk_reduce_kernel
};
struct NtPlan {
  bool ok;  // false: the fused epilogue does not qualify and the caller takes its two-launch path (always true for NT_EPI_NONE)
  NtKernel kernel;
  int tile;                 // index into kNtTiles (persistent kernels)
  int tm, tn, grid;         // tile rows, tile columns, workgroups
  int rfull, nchunks, L;    // HybridArgs (the plain schedule is {tm, 0, 1})
  size_t workspace_bytes;   // fp32 slabs of the hybrid schedule, 0 for every other kernel
};

// Hybrid plan for the 256x256 NT kernel: whole-K tiles for the full rounds, stream-K over the remaining tile rows (the work items are
// described at HybridArgs in gemm_big.hip): fills rfull / nchunks / L / workspace_bytes of *p.  Returns false when the plain schedules are
// at least as good (or the shape does not qualify).
static inline bool nt_hybrid_plan(int64_t M, int64_t N, int64_t K, int slots, const GemmPlanEnv& env, NtPlan* p) {
  if (env.nt_no_hybrid) return false;
  const bool mk = env.nt_hybrid_min_k >= 0;  // tests / A-B runs lower the thresholds
  // measured (profiles/r01_kbench_run18*): the fp32 slab traffic (~40 us) only pays off for long K.  Round 3 lowered the threshold to 2048
  // while CUs are reserved for RCCL because the plain alternative was then the 128x128 kernel (the 0.85 cliff); with the shared tile policy
  // the alternative is the persistent 256x256 kernel on two ragged rounds, which beats the hybrid at K = 2048 ... 4096 under an 8- and a
  // 16-CU reserve (profiles/r05_kbench_variants.txt: fc2 fwd 97 vs 115 us, dX qkv 108 vs 134, dX fc1 187 vs 197) - only lm_head's dX
  // (K = 50304) still gains (2004 vs 2089 us under 16 reserved CUs)
  const int64_t min_k = mk ? env.nt_hybrid_min_k : 8192, min_l = mk ? 2 : 8;
  if (K % 64 != 0 || N % 8 != 0 || M < 2048 || N < 256 || K < min_k) return false;
  const int64_t R = plan_cdiv(M, 256), Cn = plan_cdiv(N, 256), tiles = R * Cn, nkt = K / 64;
  if (tiles <= slots) return false;                          // single partial round: nothing to balance
  if (round_efficiency(tiles, slots) >= 0.9) return false;  // plain 256x256 is already well packed
  // ... or a narrower plain tile is (lm_head dX on the whole chip: 4 x 192 columns = exactly two rounds; in the step that beats the
  // hybrid's slab traffic by 0.5 % end to end, round 2).  The same per-tile rates as the automatic policy.
  double e_plain;
  nt_pick_tile(M, N, slots, &e_plain);
  if (!mk && e_plain >= 0.9) return false;
  const int64_t rf = ((tiles / slots) * slots) / Cn;        // whole tile rows inside the full rounds
  const int64_t rem = (R - rf) * Cn;
  if (rem <= 0 || rf <= 0) return false;
  const int64_t total = rem * nkt;
  const int64_t L = plan_cdiv(total, slots);
  if (L < min_l || L * 10 > nkt * 9) return false;  // too short to amortise a prologue / no round saved
  p->rfull = (int)rf;
  p->L = (int)L;
  p->nchunks = (int)plan_cdiv(total, L);
  const int64_t nslabs = (nkt - 1) / L + 2;  // pieces a tile can be cut into
  p->workspace_bytes = (size_t)nslabs * (size_t)(M - rf * 256) * (size_t)N * sizeof(float);
  return true;
}

// variant: 0 automatic | 1 / 2 the 128x128 register-staged / LDS-DMA kernel | 4 / 5 / 6 / 7 the persistent kernel on 256x256 / 256x192 /
// 256x128 / 128x192 tiles (what the automatic policy picks from) | 3 = 4.  The entry point has validated variant against the shape.
// Epilogues: ROPE and SCORE take the tile NONE picks without a workspace (never the hybrid) and do not qualify when NONE would use a
// 128x128 kernel; GLU / GLUB (N = the accumulator columns, 2h / h) run on the 256x256 tile only, whatever its efficiency.
static inline NtPlan nt_plan(int64_t M, int64_t N, int64_t K, int64_t ldc, int c_dtype, int variant, bool have_workspace, NtEpilogue epilogue,
                             int slots, const GemmPlanEnv& env) {
  NtPlan p{};
  p.ok = true;
  auto persistent = [&](int tile) {
    p.kernel = NT_PERSISTENT;
    p.tile = tile;
    p.tm = (int)plan_cdiv(M, kNtTiles[tile].bm);
    p.tn = (int)plan_cdiv(N, kNtTiles[tile].bn);
    p.grid = p.tm * p.tn < slots ? p.tm * p.tn : slots;
    p.rfull = p.tm;
    p.nchunks = 0;
    p.L = 1;
  };
  if (epilogue == NT_EPI_GLU || epilogue == NT_EPI_GLUB) {
    p.ok = !env.gemm_v1 && K % 64 == 0 && N % 256 == 0 && M >= 512;
    if (p.ok) persistent(0);
    return p;
  }
  const bool dma_ok = variant >= 2 || (variant == 0 && !env.gemm_v1 && nt_dma_shape(N, K, ldc));
  if (variant >= 3) {
    for (int i = 0; i < 4; ++i)
      if (kNtTileVariant[i] == (variant == 3 ? 4 : variant)) persistent(i);
    return p;
  }
  if (variant == 0 && dma_ok && c_dtype == 0) {
    // long K with a badly quantised tile count (lm_head dX: 384 tiles on 256 CUs): whole-K tiles for the full rounds + stream-K
    // over the remaining tile rows (needs the caller's fp32 workspace)
    if (have_workspace && epilogue == NT_EPI_NONE && nt_hybrid_plan(M, N, K, slots, env, &p)) {
      p.kernel = NT_HYBRID;
      p.tm = (int)plan_cdiv(M, 256);
      p.tn = (int)plan_cdiv(N, 256);
      const int nitems = p.rfull * p.tn + p.nchunks;
      p.grid = nitems < slots ? nitems : slots;
      return p;
    }
    // when every persistent shape quantises badly (e.g. odd slot counts while CUs are reserved for RCCL) the hardware-scheduled 128x128
    // LDS-DMA kernel is the better choice
    double eff;
    const int tile = nt_pick_tile(M, N, slots, &eff);
    if (M >= 512 && N >= 128 && eff >= nt_dma128_eff(M, N, slots)) {
      persistent(tile);
      return p;
    }
  }
  p.ok = epilogue == NT_EPI_NONE;
  p.kernel = dma_ok ? NT_DMA128 : NT_REG128;
  p.tm = (int)plan_cdiv(M, 128);
  p.tn = (int)plan_cdiv(N, 128);
  p.grid = p.tm * p.tn;
  return p;
}

// ---------------------------------------------------------------------------------------------
// TN
// ---------------------------------------------------------------------------------------------
// split count of the 128x128 kernels
static inline int tn_splits(int64_t M, int64_t N, int64_t K) {
  // The DMA kernels run 2 workgroups per CU (512 slots on 256 CUs): aim for just under 2 full rounds.
  const int64_t tiles = plan_cdiv(M, 128) * plan_cdiv(N, 128);
  if (tiles >= 512) return 1;
  int64_t s = 1024 / tiles;
  const int64_t max_by_k = K / 512 > 0 ? K / 512 : 1;  // keep >= 512 contraction rows per slab
  if (s > max_by_k) s = max_by_k;
  if (s > 32) s = 32;
  return (int)(s < 1 ? 1 : s);
}

// Plan for the persistent 256x256 TN kernel: returns false when it should not be used.  rfull = tile rows done without split.
static inline bool tn_big_plan(int64_t M, int64_t N, int64_t K, int64_t slots, int* splits, int* rfull) {
  if (K % 64 != 0 || M < 256 || N < 256) return false;
  const int64_t R = plan_cdiv(M, 256), Cn = plan_cdiv(N, 256), tiles = R * Cn;
  const int64_t max_by_k = K / 512 > 0 ? K / 512 : 1;  // >= 8 K-tiles per item
  int64_t rf = 0, s = 1;
  if (tiles < slots) {
    s = slots / tiles;
  } else {
    rf = ((tiles / slots) * slots) / Cn;
    const int64_t rem = (R - rf) * Cn;
    s = rem > 0 ? slots / rem : 1;
  }
  if (s > max_by_k) s = max_by_k;
  if (s < 1) s = 1;
  *splits = (int)s;
  *rfull = (int)rf;
  return true;
}

enum TnKernel { TN_REG128, TN_DMA128, TN_PERSISTENT };
// The rows from rfull * 256 on (`split_rows` of them) are split `splits` ways over K into fp32 slabs [splits][split_rows][N] that
// splitk_reduce_kernel sums into C; splits == 1: no slabs, no reduce, rfull covers every row of the persistent kernel.
struct TnPlan {
  TnKernel kernel;
  int tm, tn, grid;  // tile rows, tile columns (256x256 or 128x128), workgroups (per split for the 128x128 kernels: grid.y = splits)
  int splits, rfull, kchunk;
  int64_t split_rows;
  size_t workspace_bytes;
};
static inline TnPlan tn_plan(int64_t M, int64_t N, int64_t K, int slots, const GemmPlanEnv& env) {
  TnPlan p{};
  if (!env.tn_no_big && !env.gemm_v1 && tn_big_plan(M, N, K, slots, &p.splits, &p.rfull)) {
    p.kernel = TN_PERSISTENT;
    p.tm = (int)plan_cdiv(M, 256);
    p.tn = (int)plan_cdiv(N, 256);
    if (p.splits == 1 || M <= (int64_t)p.rfull * 256) {  // no remainder to split
      p.splits = 1;
      p.rfull = p.tm;
    }
    const int nitems = p.rfull * p.tn + (p.tm - p.rfull) * p.tn * p.splits;
    p.grid = nitems < slots ? nitems : slots;
  } else {
    p.kernel = (!env.gemm_v1 && K % 64 == 0) ? TN_DMA128 : TN_REG128;
    p.tm = (int)plan_cdiv(M, 128);
    p.tn = (int)plan_cdiv(N, 128);
    p.grid = p.tm * p.tn;
    p.splits = tn_splits(M, N, K);
    p.rfull = 0;
  }
  p.kchunk = p.splits == 1 ? (int)K : (int)(plan_cdiv(plan_cdiv(K, p.splits), 64) * 64);
  p.split_rows = p.splits > 1 ? M - (int64_t)p.rfull * 256 : 0;
  p.workspace_bytes = (size_t)p.splits * (size_t)p.split_rows * (size_t)N * sizeof(float);
  return p;
}

// ---- grouped TN: kernel arguments of gemm_tn_big_kernel<true> / tn_grouped_reduce_kernel and the plan that fills their schedule ----
#define PLM_TN_GROUP_MAX 48
// (kernel arguments: 48 problems x (operands + outputs) = 3.2 KB of the 4 KB kernarg segment)
struct TnGroup {
  const uint16_t* A[PLM_TN_GROUP_MAX];
  const uint16_t* B[PLM_TN_GROUP_MAX];
  int lda[PLM_TN_GROUP_MAX], ldb[PLM_TN_GROUP_MAX];
  int M[PLM_TN_GROUP_MAX], N[PLM_TN_GROUP_MAX], tiles_n[PLM_TN_GROUP_MAX];
  int tile_base[PLM_TN_GROUP_MAX + 1];  // first global tile of each problem; [count] = number of tiles
  int count;
  int n_full;  // tiles 0 .. n_full-1 take the whole contraction and write C directly (whole rounds of the persistent grid)
  int splits;  // the remaining tiles are cut `splits` ways over K (L K-tiles each): items n_full + split * n_rem + r, split-major so
  int L;       // that the workgroups of an XCD share a split's A / B panels in L2; pieces go to ws[split * n_rem + r][256][256]
};
struct TnGroupOut {
  float* C[PLM_TN_GROUP_MAX];
  const float* alpha[PLM_TN_GROUP_MAX];
  int ldc[PLM_TN_GROUP_MAX];
  int accumulate[PLM_TN_GROUP_MAX];
};

// fills the shape and schedule fields of *g; *workspace_bytes = the dense 256x256 fp32 blocks of the split tiles.  false: unsupported shapes
static inline bool tn_group_plan(const int64_t* Ms, const int64_t* Ns, int count, int64_t K, int slots, TnGroup* g, size_t* workspace_bytes) {
  if (count < 1 || count > PLM_TN_GROUP_MAX || K % 64 != 0 || K < 64) return false;
  int base = 0;
  for (int p = 0; p < count; ++p) {
    if (Ms[p] < 8 || Ns[p] < 8 || Ms[p] % 8 != 0 || Ns[p] % 8 != 0) return false;
    g->M[p] = (int)Ms[p];
    g->N[p] = (int)Ns[p];
    g->tiles_n[p] = (int)plan_cdiv(Ns[p], 256);
    g->tile_base[p] = base;
    base += (int)(plan_cdiv(Ms[p], 256) * plan_cdiv(Ns[p], 256));
  }
  g->tile_base[count] = base;
  g->count = count;
  const int64_t nkt = K / 64;
  // whole-K tiles for the full rounds; the remainder is split over K with the count that fills its rounds best (>= 8 K-tiles per
  // piece, mild bias against slab traffic).  Fewer than `slots` tiles: everything is remainder (plain split-K).
  const int nfull = (base / slots) * slots, nrem = base - nfull;
  int best = 1;
  if (nrem > 0) {
    double best_cost = 1e30;
    for (int sp = 1; sp <= 32 && (sp == 1 || nkt / sp >= 8); ++sp) {
      const int64_t L = plan_cdiv(nkt, sp);
      const int64_t rounds = plan_cdiv((int64_t)sp * nrem, slots);
      const double cost = (double)(rounds * L) * (1.0 + 0.01 * (sp - 1));  // K-tiles of wall time for the remainder
      if (cost < best_cost - 1e-9) {
        best_cost = cost;
        best = sp;
      }
    }
  }
  g->n_full = nfull;
  g->splits = nrem > 0 ? best : 0;
  g->L = (int)plan_cdiv(nkt, best);
  *workspace_bytes = (size_t)(nrem > 0 ? best * nrem : 0) * 65536 * sizeof(float);
  return (int64_t)base * nkt < (1ll << 30);
}
