// The plain attention family's LDS tile image and fragment reads (attn_generic.hip: head dims 32 / 128 with causal / document masks;
// attn_masked.hip: head dims 32 / 64 / 128 with bit-packed dense masks).  A template on the head dim, so it does not include attn_common.h
// (whose HD macro is the tuned family's 64).
#pragma once
#include "plm_fp8.h"

#define GLOG2E 1.4426950408889634f

template <int HD>
struct GenTile {
  static constexpr int ROWB = HD * 2 + 16;  // bytes per tile row in LDS: 16 bytes of padding spread the rows over the banks
  static constexpr int BYTES = 64 * ROWB;
  // the whole workgroup (256 threads) copies rows row0 .. row0 + 63 (clamped to last_row) of a [*, ld] bf16 matrix at column col0
  static __device__ __forceinline__ void load(char* tile, const uint16_t* src, int64_t ld, int row0, int last_row, int tid) {
    constexpr int CPR = HD / 8;  // 16-byte chunks per row
    for (int c = tid; c < 64 * CPR; c += 256) {
      const int r = c / CPR, k = c - r * CPR;
      *reinterpret_cast<bf16x8_t*>(tile + r * ROWB + k * 16) = ld_bf16x8(src + (int64_t)min(row0 + r, last_row) * ld + k * 8);
    }
  }
  // the same image from an FP8 cache (plm_fp8.h): codes = the row's e4m3 bytes at this head's first column,
  // scales = the row's E8M0 bytes at this head's first 16-block, both [*, ld] bytes.  A 16-byte LDS chunk is 8 codes times their block's
  // scale, exact in bf16; the row clamp is load's.
  static __device__ __forceinline__ void load(char* tile, const uint8_t* codes, const uint8_t* scales, int64_t ld, int row0, int last_row,
                                              int tid) {
    constexpr int CPR = HD / 8;
    for (int c = tid; c < 64 * CPR; c += 256) {
      const int r = c / CPR, k = c - r * CPR;
      const int64_t ro = (int64_t)min(row0 + r, last_row) * ld;
      const u32x2_t w = *reinterpret_cast<const u32x2_t*>(codes + ro + k * 8);
      *reinterpret_cast<bf16x8_t*>(tile + r * ROWB + k * 16) = kv8_deq8_bf16(w, scales[ro + (k >> 1)]);
    }
  }
  // A operand, i = tile row (lane & 31), k = head dims ks*16 + hi*8 .. + 7
  static __device__ __forceinline__ bf16x8_t rows(const char* tile, int row, int ks, int hi) {
    return *reinterpret_cast<const bf16x8_t*>(tile + row * ROWB + (ks * 16 + hi * 8) * 2);
  }
  // A operand, i = head dim db*32 + (lane & 31), k-slot e of lane half hi = tile row rbase + (e & 3) + 8 (e >> 2)  (see frag_cols, attn_common.h)
  static __device__ __forceinline__ bf16x8_t cols(const char* tile, int db, int rbase, int lane) {
    const int ib = (lane >> 4) & 1, t16 = lane & 15;
    const int col = db * 32 + ib * 16 + (t16 & 3) * 4;
    const int row = rbase + (t16 >> 2);
    return join_tr(lds_read_tr16(tile + row * ROWB + col * 2), lds_read_tr16(tile + (row + 8) * ROWB + col * 2));
  }
};

__device__ __forceinline__ void gzero16(f32x16_t& v) {
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = 0.f;
}
