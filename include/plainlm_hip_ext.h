/* plainlm_hip_ext.h — additions to the C ABI of libplainlm_hip.so (MI355X / gfx950 only).
 *
 * A second public header next to plainlm_hip.h, for one reason: the footprint and binding tests keep a table with one row per
 * function of plainlm_hip.h, and entry points added by a change that may not edit those tables are declared here, with a table
 * (plainlm_amd/_lib.py: EXT_SIGNATURES) and footprint cases (tests/test_footprint_predict_gpu.py) of their own.  The conventions
 * are those of plainlm_hip.h (device pointers owned by the caller, `stream` a hipStream_t passed as void*, asynchronous, never
 * allocating, 0 = ok, PLM_E_* < 0 and plm_last_error_string() otherwise); plm_version() does not move for these additions.  A later
 * change that is free to touch the tables can fold this file into plainlm_hip.h.
 */
#ifndef PLAINLM_HIP_EXT_H
#define PLAINLM_HIP_EXT_H

#include "plainlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- prediction head -----
 * Per row of l = bf16(Y[M,K] W[V,K]^T) - the logits plm_gemm_bf16_nt would store and plm_head_score_bf16 reduces: same tile shape,
 * same K order, same rounding - WITHOUT ever storing them:
 *   pred    int64[M]  column of the largest logit, the lowest column among equal ones; always in [0, V), also for a row with NaN
 *   logp    fp32[M]   log softmax(l)[pred] = max(l) - lse  (<= 0)
 *   entropy fp32[M]   lse - sum_i softmax(l)_i l_i, in nats                                   (may be NULL)
 *   nll     fp32[M]   lse - l[target], 0 for a target outside [0, V)                          (may be NULL; needs targets)
 *   lse     fp32[M]   logsumexp(l)                                                            (may be NULL)
 * nll and lse carry the bits plm_head_score_bf16 returns for the same operands.  targets int64[M] may be NULL (then nll must be).
 * The persistent NT kernel reduces every output tile to one 16-byte record per row (max, sum-exp, sum e^(l-max) (l-max), column of
 * the first maximum) and a second launch combines a row's records in a fixed order.  No gradient is produced.
 * workspace: plm_head_predict_workspace_bytes(M, V, K) bytes (about M * ceil(V / 128) * 16), 16-byte aligned, caller-owned.
 * NULL pointers, K % 64 != 0, row strides that are not multiples of 8, Y / W that are not 16-byte aligned give PLM_E_INVALID and a
 * short workspace PLM_E_WORKSPACE before anything is launched.  Shapes that plm_gemm_bf16_nt serves with a 128x128 kernel (M < 512,
 * V % 8 != 0) go through that kernel, 256 rows of logits at a time inside the workspace.  Deterministic (no atomics). */
size_t plm_head_predict_workspace_bytes(int64_t M, int64_t V, int64_t K);
int plm_head_predict_bf16(const uint16_t* Y, int64_t ldy, const uint16_t* W, int64_t ldw, const int64_t* targets, int64_t* pred,
                          float* logp, float* entropy, float* nll, float* lse, int64_t M, int64_t V, int64_t K, void* workspace,
                          size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PLAINLM_HIP_EXT_H */
