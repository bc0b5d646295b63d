// What the GEMM kernel files (gemm.hip, gemm_big.hip) export to the entry points (gemm_api.hip): launch functions that execute a plan of
// gemm_plan.h.  They check nothing: shapes, pointers, workspace sizes and the choice of kernel are the entry points' business.
#pragma once

#include "gemm_plan.h"
#include "plm_device.h"

// epilogue operands of gemm_nt_big_kernel (the epilogues are described above the kernel)
struct EpiArgs {
  uint16_t* act;        // GLU: activation output [M, N/2];  GLUB: the saved fc1 output [M, 2N] (read-only)
  int64_t ldact;
  const float* rcos;    // ROPE: fp32 [T, 32] tables
  const float* rsin;
  int T, rope_cols;
  // SCORE: forward-only scoring head (see the SCORE epilogue in the kernel).  C is not written.
  const int64_t* targets;  // [M]
  float* part;             // [tiles_n][M] (max, sum-exp) pairs, one per row and tile column
  float* xt;               // [M] the bf16-rounded target logit of every row whose target is a valid column
  // SCORE, prediction mode (plm_head_predict_bf16): non-null selects it.  The per-row record grows to
  // (max, sum-exp, u = sum e^(x-max) (x-max), column of the first maximum as int bits) and goes HERE instead of `part`; targets may be null.
  float* part4;            // [tiles_n][M] 16-byte records
};

struct GemmOperands {
  const uint16_t* A;
  int64_t lda;
  const uint16_t* B;
  int64_t ldb;
  void* C;  // NT: bf16 (fp32 for the 128x128 kernels with c_dtype 1); TN: fp32
  int64_t ldc, M, N, K;
  const float* alpha_dev;
};

// gemm.hip: the 128x128 kernels
void plm_launch_gemm_nt_128(const NtPlan& p, const GemmOperands& o, int c_dtype, int accumulate, hipStream_t s);
void plm_launch_gemm_tn_128(const TnPlan& p, const GemmOperands& o, int accumulate, float* slabs, hipStream_t s);
void plm_launch_splitk_reduce(const TnPlan& p, const GemmOperands& o, int accumulate, float* slabs, hipStream_t s);  // after either TN kernel when p.splits > 1

// gemm_big.hip: the persistent kernels
void plm_launch_gemm_nt_persistent(const NtPlan& p, NtEpilogue epilogue, const GemmOperands& o, float* slabs, const EpiArgs& ea, hipStream_t s);
void plm_launch_gemm_tn_persistent(const TnPlan& p, const GemmOperands& o, int accumulate, float* slabs, hipStream_t s);
void plm_launch_gemm_tn_grouped(const TnGroup& g, const TnGroupOut& out, int64_t K, float* ws, int slots, hipStream_t s);
void plm_launch_head_score_combine(const float* part, const float* xt, const int64_t* targets, float* nll, float* lse, int64_t M, int64_t V, int ntc,
                                   hipStream_t s);
void plm_launch_head_score_rows(const uint16_t* logits, int64_t ld, const int64_t* targets, float* nll, float* lse, int64_t rows, int64_t V,
                                hipStream_t s);
// outputs of the prediction head, one element per row; all but pred / logp may be null (nll needs targets)
struct HeadPredictOut {
  int64_t* pred;
  float *logp, *entropy, *nll, *lse;
};
void plm_launch_head_predict_combine(const float* part4, const float* xt, const int64_t* targets, const HeadPredictOut& out, int64_t M, int64_t V,
                                     int ntc, hipStream_t s);
void plm_launch_head_predict_rows(const uint16_t* logits, int64_t ld, const int64_t* targets, const HeadPredictOut& out, int64_t rows, int64_t V,
                                  hipStream_t s);
