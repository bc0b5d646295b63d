/* plainlm_hip_sample.h — on-device sampling for KV-cached generation (libplainlm_hip.so, MI355X / gfx950 only).
 *
 * A fourth public header, for the reason plainlm_hip_ext.h and plainlm_hip_gen.h are the second and third: the binding and footprint
 * tests pin the exact function lists of the three older headers (64 / 2 / 3 functions), so none of them may gain a declaration from a
 * change that leaves those tests as they are.  Table: plainlm_amd/_lib.py SAMPLE_SIGNATURES; footprint cases:
 * tests/test_footprint_sample_gpu.py.  The conventions are those of plainlm_hip.h (device pointers owned by the caller, `stream` a
 * hipStream_t passed as void*, asynchronous, never allocating, 0 = ok, PLM_E_* < 0 and plm_last_error_string() otherwise; every argument
 * check comes before any HIP call); plm_version() does not move for this addition.
 */
#ifndef PLAINLM_HIP_SAMPLE_H
#define PLAINLM_HIP_SAMPLE_H

#include "plainlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- temperature / top-k / top-p sampling of one token per row -----
 * logits bf16 [B, ld] (ld >= V; any 2-byte aligned base and any ld: columns >= V are never loaded); u fp32 [B], one uniform per row,
 * clamped on the device (NaN or negative -> 0, >= 1 -> the largest float below 1).  One launch, one workgroup per row, no workspace;
 * row b's outputs depend on row b and u[b] alone, and the same inputs give the same bits on every run (integer histograms and 64-bit
 * fixed-point sums only: no result depends on the order in which anything arrives).
 *
 * The rule, in this order.  A NaN, -inf (or +inf: outside the contract) logit has weight 0, is never kept and never chosen.
 *   temperature  w_i = exp((x_i - x_max) / temperature), fp32; x_max the largest finite logit of the row.
 *   top-k        by VALUE: with v_k the top_k-th largest value, every i with x_i >= v_k stays - all ties with the k-th value included.
 *                top_k = 0 or top_k >= V: off.
 *   top-p        by VALUE CLASS: mass(t) = sum of w_i over the top-k survivors with x_i >= t, as a share of their total; t* is the
 *                largest value present with mass(t*) >= top_p; every survivor with x_i >= t* stays.  Equal logits go in or out together;
 *                the maximum's class always stays.  top_p = 1: off.
 *   draw         over the kept columns in ascending index order, C_i the running sum of w, Z the last C: the lowest kept i with
 *                C_i > u * Z.
 * Outputs: tok int64 [B], always in [0, V); logp fp32 [B] = log softmax(x)[tok] over all V raw logits at temperature 1 (the model's
 * log-probability); unless NULL, n_kept int32 [B] = the size of the kept set and cutoff fp32 [B] = its lowest raw logit.  A row without
 * any finite logit gives tok = 0, n_kept = 0, logp = cutoff = NaN.
 * PLM_E_INVALID before anything is launched for: a NULL pointer (n_kept and cutoff excepted), B < 1, V < 1 or V >= 2^31, ld < V, a
 * logits base that is not 2-byte aligned, a temperature that is not finite or <= 0, top_k < 0, top_p outside (0, 1]. */
int plm_sample_logits_bf16(const uint16_t* logits, int64_t ld, const float* u, float temperature, int64_t top_k, float top_p,
                           int64_t* tok, float* logp, int32_t* n_kept, float* cutoff, int64_t B, int64_t V, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PLAINLM_HIP_SAMPLE_H */
