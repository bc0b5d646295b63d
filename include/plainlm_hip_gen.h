/* plainlm_hip_gen.h — the generation entry points of libplainlm_hip.so (MI355X / gfx950 only).
 *
 * A third public header, for the reason plainlm_hip_ext.h is the second: the binding and footprint tests pin the exact function lists
 * of plainlm_hip.h (64 functions, _lib.SIGNATURES) and of plainlm_hip_ext.h (the two head-predict functions, _lib.EXT_SIGNATURES), so
 * neither may gain a declaration from a change that leaves those tests as they are.  The KV-cache entry points are declared here, with a
 * table (plainlm_amd/_lib.py: GEN_SIGNATURES) and footprint cases (tests/test_footprint_decode_gpu.py) of their own.  The conventions are
 * those of plainlm_hip.h (device pointers owned by the caller, `stream` a hipStream_t passed as void*, asynchronous, never allocating,
 * 0 = ok, PLM_E_* < 0 and plm_last_error_string() otherwise; every argument check comes before any HIP call); plm_version() does not
 * move for these additions.  A later change that is free to touch the tables can fold this file into plainlm_hip.h.
 */
#ifndef PLAINLM_HIP_GEN_H
#define PLAINLM_HIP_GEN_H

#include "plainlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- KV-cached generation -----
 * Cache layout: one bf16 buffer per layer, kv[B, Tmax, ld_kv] (ld_kv >= 2*nh*hd, a multiple of 8; sequence b starts at b * Tmax * ld_kv).
 * Row (b, j) holds the k | v column blocks of token j of sequence b: columns [nh*hd, 3*nh*hd) of that layer's ROTATED qkv row, the bits
 * plm_qkv_rope_bf16 wrote.  head_dim is 32, 64 or 128.
 *
 * plm_kv_append_rope: one token per sequence.  qkv bf16 [B, ld_qkv] is the UN-rotated projection (q | k | v, 3*nh*hd columns); pos
 * int32[B]; rope_cos / rope_sin fp32 [rope_T, hd/2].  For every sequence with 0 <= pos[b] < min(Tmax, rope_T): q and k are rotated at
 * position pos[b] with the arithmetic of plm_rope_qk (same bits), rotated q goes to q_out bf16 [B, nh*hd], rotated k and the untouched v
 * to kv[b, pos[b], 0 : 2*nh*hd].  Any other pos[b] writes nothing for that sequence and sets the caller-zeroed status[0] to 1 (the
 * convention of plm_attn_doc_start_from_mask).  One launch.  qkv, q_out, kv and the tables must be 16-byte aligned. */
int plm_kv_append_rope(const uint16_t* qkv, int64_t ld_qkv, const int32_t* pos, const float* rope_cos, const float* rope_sin,
                       int64_t rope_T, uint16_t* q_out, uint16_t* kv, int64_t ld_kv, int32_t* status, int64_t B, int64_t Tmax, int64_t nh,
                       int64_t hd, void* stream);

/* plm_attn_decode: attention of one (rotated) query row per sequence over its cache.  q bf16 [B, nh*hd]; lens int32[B], clamped to
 * [0, Tmax]: sequence b, head h attends keys 0 .. lens[b]-1, and cache rows at and beyond lens[b] are never read.  Writes out bf16
 * [B, nh*hd] and, unless NULL, lse fp32 [B, nh]: the base-2 log-sum-exp of the scaled scores, plm_attn_fwd's convention, comparable with
 * row lens[b]-1 of a full causal forward.  lens[b] == 0 gives out = 0 and lse = +INFINITY (the masked kernels' rule for a row with no key).
 * Flash-decoding: a (B*nh) x S grid walks S contiguous key ranges per (sequence, head) and leaves fp32 partials (max, sum, acc[hd]) in the
 * workspace; a second launch combines them in split order.  No atomics: bit-reproducible, and for a fixed S independent of the other
 * sequences of the batch.  splits: 0 = automatic (a function of B, nh, Tmax and the CU count only - lens is never read back), 1..64
 * forced.  workspace: plm_attn_decode_workspace_bytes(B, nh, hd, Tmax, splits) bytes for the same splits argument, 16-byte aligned,
 * caller-owned (the query returns 0 for arguments the launch refuses).  NULL pointers (lse excepted), a head_dim other than 32 / 64 /
 * 128, bases that are not 16-byte aligned, splits outside 0..64 give PLM_E_INVALID and a short workspace PLM_E_WORKSPACE before anything
 * is launched. */
size_t plm_attn_decode_workspace_bytes(int64_t B, int64_t nh, int64_t hd, int64_t Tmax, int splits);
int plm_attn_decode(const uint16_t* q, const uint16_t* kv, int64_t ld_kv, const int32_t* lens, uint16_t* out, float* lse, int64_t B,
                    int64_t Tmax, int64_t nh, int64_t hd, int splits, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PLAINLM_HIP_GEN_H */
