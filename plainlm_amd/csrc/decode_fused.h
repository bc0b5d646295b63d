// What the fused layer families share (decode_fused.hip: the skinny-M stages of DESIGN.md sections 17 and 18; layer_wide.hip: the wide
// stages of section 27): the stage arguments, the pair helpers of the epilogues and the host-side checks that know no row cap.
#pragma once
#include "plm_fp8.h"

enum { DF_PRO_BF16 = 0, DF_PRO_NORM = 1 };
enum { DF_EPI_RESIDUAL = 1, DF_EPI_GLU = 2, DF_EPI_SILU = 3, DF_EPI_RELU_SQ = 4, DF_EPI_QKV_ROWS = 5, DF_EPI_QKV_ROWS_KV8 = 6, DF_EPI_QKV_ROWS_PAGED = 7, DF_EPI_QKV_PACKED_PAGED = 8 };

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
  const int32_t* rot0;   // [M / n] or null: the rows are rotated at rot0[b] + lens0[b] + r (a suffix cache); null: at their row
  const int32_t* depth;  // [M] or null: row r is a tree node rotated at lens0[b] + depth[b, r], stored at lens0[b] + r as ever (DESIGN.md section
                         // 22; depth[b, 0] < 0: plm_tree_plan refused the sequence, nothing of it is stored); null: at their row
  // QKV_ROWS_PAGED: kv is a pool [n_pages, PLM_KV_PAGE_ROWS, ld_kv], row t of sequence b lives in page
  // table[b, t / 64]; Tmax = max_pages * 64
  const int32_t* table;  // [M / n, max_pages]
  int max_pages, n_pages;
  // QKV_PACKED_PAGED: QKV_ROWS_PAGED with the packed row -> (sequence, position) map in place of m / n, m % n:
  // row m is row m - cu_rows[b] of sequence b = row_seq[m] when 0 <= b < B and cu_rows[b] <= m < cu_rows[b + 1], else padding
  const int32_t* cu_rows;  // [B + 1]
  const int32_t* row_seq;  // [M]
  int B;
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

#define DF_MAX_DIM 65536  // K and N of a stage: far above any model this library serves, keeps every index inside 32 bits

static bool df_aligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr,
                       const void* f = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d) |
           reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(f)) & 15) == 0;
}

// A paged cache's operands: the qkv stage stores through the table into the pool that stands in kv's place, the
// attention stage walks Lcap keys of the table.  live: the decode layer's n_new (0: an idle slot appends nothing), may be null.
struct DfPaged {
  const int32_t* table;
  const int32_t* live;
  int64_t max_pages, n_pages, Lcap;
  // a ragged step: R packed rows of B sequences in NT tiles; null / 0 otherwise
  const int32_t* cu_rows = nullptr;
  const int32_t* row_seq = nullptr;
  int64_t R = 0, B = 0, NT = 0;
};

// what the packed-row words add to a stage's refusals (plm_kv_paged_append_rope_packed's)
static int df_check_packed(const char* fn, const DfPaged& pg, const int32_t* lens0) {
  PLM_REQUIRE(pg.cu_rows && pg.row_seq && lens0, "%s: null pointer", fn);
  PLM_REQUIRE(pg.B >= 1 && pg.B <= (1 << 20), "%s: bad shape B=%ld sequences (1 <= B <= 2^20)", fn, (long)pg.B);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(pg.cu_rows) | reinterpret_cast<uintptr_t>(pg.row_seq) | reinterpret_cast<uintptr_t>(lens0)) & 3) == 0,
              "%s: lens0, cu_rows and row_seq must be 4-byte aligned", fn);
  return PLM_OK;
}

static int df_check_paged(const char* fn, const DfPaged& pg, bool attend) {
  PLM_REQUIRE(pg.table, "%s: null pointer", fn);
  PLM_REQUIRE((reinterpret_cast<uintptr_t>(pg.table) & 3) == 0, "%s: the table must be 4-byte aligned", fn);
  PLM_REQUIRE(pg.max_pages > 0 && pg.max_pages < (1 << 18) && pg.n_pages > 0 && pg.n_pages < (1 << 24),
              "%s: bad shape max_pages=%ld n_pages=%ld (max_pages < 2^18, n_pages < 2^24)", fn, (long)pg.max_pages, (long)pg.n_pages);
  PLM_REQUIRE(!attend || (pg.Lcap >= 1 && pg.Lcap <= pg.max_pages * PLM_KV_PAGE_ROWS), "%s: Lcap=%ld outside [1, max_pages * %d = %ld]", fn,
              (long)pg.Lcap, PLM_KV_PAGE_ROWS, (long)(pg.max_pages * PLM_KV_PAGE_ROWS));
  return PLM_OK;
}

static size_t df_round16(size_t n) { return (n + 15) / 16 * 16; }
