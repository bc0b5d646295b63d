// What attn_cache.hip lends to attn_shared.hip: the split limits, the automatic split rule, and the launches of
// its decode split kernel and of its combine kernel over a partial layout with more splits per (sequence, head) than one launch fills.
#pragma once
#include "plm_device.h"

#define CACHE_MAX_SPLITS 64
// the automatic split rules know the device by this one number (MI355X: 256 CUs); nothing is queried, nothing is read back
#define CACHE_CUS 256

// plm_attn_decode / plm_attn_extend's automatic split count (splits == 0), or the forced one
int cache_resolve_splits(int64_t B, int64_t n, int64_t nh, int64_t Tmax, int splits);
// plm_attn_decode's shape limits
bool cache_shape_ok(int64_t B, int64_t n, int64_t nh, int64_t hd, int64_t Tmax);
// bytes of fp32 partials (m, l, acc[hd]) for B*nh*S*n (query row, split) pairs, a multiple of 16
size_t cache_ws_bytes(int64_t B, int64_t n, int64_t nh, int64_t hd, int S);

// attn_decode_split_kernel over a bf16 cache with S splits, writing the partials of (b, h, s) at index (b*nh + h) * part_stride + part_off + s
// of ws_ml [., 2] / ws_acc [., hd]
void cache_decode_partials_launch(const uint16_t* q, const uint16_t* kv, int64_t ld_kv, const int32_t* lens, float* ws_ml, float* ws_acc, int64_t B,
                                  int64_t Tmax, int64_t nh, int64_t hd, int S, int part_stride, int part_off, hipStream_t s);
// attn_cache_combine_kernel at n = 1 over S partials per (b, h).  n_new / grp (attn_tree.hip): the B rows are grp chunk rows per n_new entry,
// and a row at or beyond its entry reads no partial (out = 0, lse = +inf); without them every row is combined.  n > 1 (attn_paged.hip, grp
// == 0): the chunk form, partials [B*nh, S, n], row r of sequence b combined when r < n_new[b]
void cache_combine_launch(const float* ws_acc, const float* ws_ml, uint16_t* out, float* lse, int64_t B, int64_t nh, int64_t hd, int S, hipStream_t s,
                          const int32_t* n_new = nullptr, int grp = 0, int64_t n = 1);

// What attn_shared.hip lends to attn_tree.hip: its split rule and the launch of attn_shared_prefix_kernel - P prompts,
// G query rows each (row p*G + g of q), Sp splits into a partial layout of Stot per (query row, head), ml [., 2] then acc [., hd]
int shared_resolve_splits_p(int64_t P, int64_t G, int64_t nh, int64_t Tp_max, int splits_p);
void shared_prefix_launch(const uint16_t* q, const uint16_t* kv_p, int64_t ld_kv_p, const int32_t* lens_p, float* ws_ml, float* ws_acc, int64_t P,
                          int64_t G, int64_t Tp_max, int64_t nh, int64_t hd, int Sp, int Stot, hipStream_t s);
