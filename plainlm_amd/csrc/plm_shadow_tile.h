// The bf16 shadow pair of an fp32 matrix W [rows, cols]: dst = bf16(W) in W's layout and dst_t = bf16(W)^T [cols, ld_t], one 64 x 64
// tile per 256-thread workgroup through an LDS transposition; and the item table of the entry points that do this for a list of
// matrices in one launch.  Shared by the casts (elementwise.hip) and the shadow-emitting optimizer tail (optim.hip).
#pragma once

#include "plm_device.h"

// `quad(o)` yields the fp32 values of elements o .. o + 3 (the casts: a load; the optimizers: load - update - store).  It is called
// for quads inside the matrix only; lanes outside put zeros into the LDS tile, which the transposed store never reads back.
template <typename Quad>
__device__ __forceinline__ void shadow_tile(uint16_t* __restrict__ dst, uint16_t* __restrict__ dst_t, int64_t rows, int64_t cols,
                                            int64_t ld_t, int64_t r0, int64_t c0, Quad&& quad) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[64][72];  // [col][row], 144-byte rows (16B aligned)
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (t >> 4) + 16 * i, c = (t & 15) * 4;
    const int64_t gr = r0 + r, gc = c0 + c;
    const bool in = gr < rows && gc < cols;  // cols % 8 == 0: the four columns are in range together
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    if (in) v = quad(gr * cols + gc);
    bf16x4_t o;
    o[0] = f2bf(v[0]); o[1] = f2bf(v[1]); o[2] = f2bf(v[2]); o[3] = f2bf(v[3]);
    if (in) st_bf16x4(dst + gr * cols + gc, o);
    tile[c + 0][r] = o[0]; tile[c + 1][r] = o[1]; tile[c + 2][r] = o[2]; tile[c + 3][r] = o[3];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = (t >> 3) + 32 * i, rch = (t & 7) * 8;
    const int64_t gc = c0 + c, gr = r0 + rch;
    if (gc < cols && gr < rows) {  // rows % 8 == 0: the eight rows are in range together
      const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(&tile[c][rch]);
      st_bf16x8(dst_t + gc * ld_t + gr, v);
    }
  }
}

// Shapes of up to 56 matrices and the first workgroup of each; travels in the kernel arguments next to the caller's pointer arrays.
#define PLM_SHADOW_ITEMS_MAX 56
struct ShadowTable {
  int rows[PLM_SHADOW_ITEMS_MAX], cols[PLM_SHADOW_ITEMS_MAX], ld_t[PLM_SHADOW_ITEMS_MAX];
  int block_base[PLM_SHADOW_ITEMS_MAX + 1];  // first block of each item; [count] = number of blocks
  int count;
};

// the item this workgroup works on and the origin of its tile
__device__ __forceinline__ int shadow_locate(const ShadowTable& s, int64_t& r0, int64_t& c0) {
  int it = 0;
  for (int q = 1; q < s.count; ++q)
    if ((int)blockIdx.x >= s.block_base[q]) it = q;  // block-uniform scalar search
  const int local = blockIdx.x - s.block_base[it];
  const int tiles_x = (s.cols[it] + 63) / 64;
  r0 = (int64_t)(local / tiles_x) * 64;
  c0 = (int64_t)(local % tiles_x) * 64;
  return it;
}

// Host side of a multi-tensor entry point `who` over plm_cast_item / plm_optim_item lists: EVERY item is validated before the first
// launch (a refused list leaves all matrices as they were), then one launch per 56 items.  `check(item, i)` holds the entry point's
// own pointer rules and returns PLM_OK or the error it has set; `launch(first, n, table)` issues the kernel for items first .. first+n-1.
template <typename Item, typename Check, typename Launch>
static int shadow_items_run(const char* who, const Item* items, int count, Check&& check, Launch&& launch) {
  PLM_REQUIRE(items && count >= 1, "%s: null pointer or empty list", who);
  int64_t tiles = 0;
  for (int i = 0; i < count; ++i) {
    const Item& q = items[i];
    if (const int e = check(q, i)) return e;
    PLM_REQUIRE(q.rows > 0 && q.cols > 0 && q.rows % 8 == 0 && q.cols % 8 == 0 && q.rows < (1ll << 31) && q.cols < (1ll << 31),
                "%s: item %d: rows=%ld cols=%ld must be positive multiples of 8", who, i, (long)q.rows, (long)q.cols);
    PLM_REQUIRE(q.ld_t >= q.rows && q.ld_t % 8 == 0 && q.ld_t < (1ll << 31), "%s: item %d: ld_t=%ld must be >= rows and a multiple of 8",
                who, i, (long)q.ld_t);
    if (i % PLM_SHADOW_ITEMS_MAX == 0) tiles = 0;  // the grid of one launch
    tiles += plm_cdiv(q.rows, 64) * plm_cdiv(q.cols, 64);
    PLM_REQUIRE(tiles < (1ll << 31), "%s: too many tiles", who);
  }
  for (int first = 0; first < count; first += PLM_SHADOW_ITEMS_MAX) {
    const int n = count - first < PLM_SHADOW_ITEMS_MAX ? count - first : PLM_SHADOW_ITEMS_MAX;
    ShadowTable s{};
    int base = 0;
    for (int i = 0; i < n; ++i) {
      const Item& q = items[first + i];
      s.rows[i] = (int)q.rows; s.cols[i] = (int)q.cols; s.ld_t[i] = (int)q.ld_t;
      s.block_base[i] = base;
      base += (int)(plm_cdiv(q.rows, 64) * plm_cdiv(q.cols, 64));
    }
    s.block_base[n] = base;
    s.count = n;
    launch(first, n, s);
    PLM_CHECK_LAUNCH(who);
  }
  return PLM_OK;
}
