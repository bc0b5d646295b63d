/* plainlm_hip.h — C ABI of libplainlm_hip.so (MI355X / gfx950 only).
 *
 * plainLM has no FFI of its own: its hot path is Python calling torch ops
 * (SURVEY.md §8b).  Each entry point below therefore cites the torch call site
 * in the reference that it replaces (paths relative to the reference root).
 *
 * Conventions (identical for every function):
 *   - all pointers are DEVICE pointers owned by the caller (workspaces too);
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on
 *     that stream, never synchronises, never allocates;
 *   - bf16 tensors are passed as uint16_t* (raw bfloat16 bits), row-major;
 *   - return value: 0 = ok, <0 = error (PLM_E_*); plm_last_error_string()
 *     returns a thread-local description of the last failure on this thread;
 *   - re-entrant and thread-safe per stream (autograd's backward thread differs
 *     from the forward thread).
 */
#ifndef PLAINLM_HIP_H
#define PLAINLM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLM_OK 0
#define PLM_E_INVALID (-1)     /* bad argument / unsupported shape */
#define PLM_E_HIP (-2)         /* a HIP runtime call or launch failed */
#define PLM_E_COMM (-3)        /* RCCL failure */
#define PLM_E_WORKSPACE (-4)   /* caller-provided workspace too small */

int plm_version(void);
const char* plm_last_error_string(void);
/* The library reads its environment switches (PLM_GEMM_V1, PLM_TN_NO_BIG, PLM_NT_NO_HYBRID, PLM_NT_HYBRID_MIN_K: tests and A/B
 * runs; none is needed in production) ONCE, at its first call - no launch path calls getenv.  A process that changes one of them
 * afterwards (the test-suite does) calls this to have them read again. */
void plm_reload_env(void);

/* ---- parameter casts --------------------------------------------------
 * Replaces autocast's per-forward fp32->bf16 weight casts
 * (engine/engine.py:75,108-109).  The `_t` form also writes the transposed
 * copy dst_t[cols, ld_t] (ld_t >= rows; columns rows..ld_t are left untouched) used by the dX GEMMs. */
int plm_cast_f32_bf16(const float* src, uint16_t* dst, int64_t n, void* stream);
int plm_cast_f32_bf16_t(const float* src, uint16_t* dst, uint16_t* dst_t, int64_t rows, int64_t cols, int64_t ld_t, void* stream);
/* the `_t` cast for a whole list of weights in one launch per 56 items (every Linear of the model at the top of a step); every item
 * is validated before the first launch */
typedef struct plm_cast_item {
  const float* src; /* fp32 [rows, cols] */
  uint16_t* dst;    /* bf16 [rows, cols] */
  uint16_t* dst_t;  /* bf16 [cols, ld_t], columns 0..rows-1 written */
  int64_t rows, cols, ld_t;
} plm_cast_item;
int plm_cast_f32_bf16_t_multi(const plm_cast_item* items, int count, void* stream);

/* ---- embedding (models/transformer.py:94,110) --------------------------
 * fwd: out[m,:] = W[ids[m],:]           ids int64[M], W fp32[V,d], out fp32[M,d]
 * bwd: dW[ids[m],:] += dout[m,:]        (atomic fp32 adds; dW must be initialised) */
int plm_embed_fwd(const int64_t* ids, const float* W, float* out, int64_t M, int64_t d, int64_t V, void* stream);
int plm_embed_bwd(const int64_t* ids, const float* dout, float* dW, int64_t M, int64_t d, int64_t V, void* stream);
/* Deterministic variant without atomics: stable radix sort of the ids, then every vocabulary row is written exactly once as
 * the sum of its tokens' rows in increasing token order (rows without tokens: zeros when accumulate == 0, untouched
 * otherwise).  Needs M <= 65536 and V < 65536 and a workspace of plm_embed_bwd_workspace_bytes(M, V) bytes (0 = shape not
 * supported, use plm_embed_bwd).  With accumulate == 0 dW does not have to be cleared first. */
size_t plm_embed_bwd_workspace_bytes(int64_t M, int64_t V);
int plm_embed_bwd_sorted(const int64_t* ids, const float* dout, float* dW, int64_t M, int64_t d, int64_t V, int accumulate,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- RMSNorm (+ residual add) (models/components.py:16-28, transformer.py:81-82)
 * fwd:  r = x (+ branch if branch != NULL)          x fp32[M,d], branch bf16[M,d]
 *       if xout != NULL: xout = r                    fp32[M,d]  (may alias x)
 *       rstd[m] = rsqrt(mean(r^2) + eps)             fp32[M]
 *       y = bf16((r * rstd) * w)                     bf16[M,d]
 * bwd:  a = dy * w ; dxn = rstd*a - x*rstd^3*mean(a*x)
 *       dx = (gin ? gin : 0) + dxn                   fp32[M,d]  (may alias gin)
 *       if dx_bf16 != NULL: dx_bf16 = bf16(dx)
 *       dw_partial[blk,:] = sum over the block's rows of dy*x*rstd   fp32[nblk,d]
 *       nblk = plm_rmsnorm_bwd_blocks(M); reduce with plm_colsum_f32. */
int plm_rmsnorm_fwd(const float* x, const uint16_t* branch, float* xout, const float* w, uint16_t* y, float* rstd,
                    int64_t M, int64_t d, float eps, void* stream);
int64_t plm_rmsnorm_bwd_blocks(int64_t M);
int plm_rmsnorm_bwd(const uint16_t* dy, const float* x, const float* w, const float* rstd, const float* gin,
                    float* dx, uint16_t* dx_bf16, float* dw_partial, int64_t M, int64_t d, void* stream);
/* out[j] (+)= sum_r part[r, j]; accumulate != 0 adds into out. */
int plm_colsum_f32(const float* part, float* out, int64_t rows, int64_t cols, int accumulate, void* stream);
/* the same reduction for a whole list of partial buffers in ONE launch (all RMSNorm weight gradients of a backward pass:
 * 25 at the 160M size, each a few microseconds of launch-bound work); every item has the same rows x cols */
typedef struct plm_colsum_item {
  const float* part; /* fp32 [rows, cols] */
  float* out;        /* fp32 [cols] */
  int accumulate;
} plm_colsum_item;
int plm_colsum_f32_multi(const plm_colsum_item* items, int count, int64_t rows, int64_t cols, void* stream);

/* ---- SwiGLU gate (models/components.py:55-56) ---------------------------
 * u bf16[M,2h] = fc1 output, x = u[:, :h], z = u[:, h:]
 * fwd: out = bf16(bf16(silu(x)) * z)                          bf16[M,h]
 * bwd: du[:, :h] = d/dx, du[:, h:] = d/dz (bf16 autograd chain of the reference) */
int plm_swiglu_fwd(const uint16_t* u, uint16_t* out, int64_t M, int64_t h, void* stream);
int plm_swiglu_bwd(const uint16_t* dout, const uint16_t* u, uint16_t* du, int64_t M, int64_t h, void* stream);
/* The activations of the reference's two plain MLP classes (models/components.py:31-40 `MLP` = fc2(silu(fc1 x)); :59-70 `MLPReluSquared` =
 * fc2(relu(fc1 x)^2); models/transformer.py:26 MLP_CLASSES), element-wise over n = M * h bf16 values (n % 8 == 0, 16-byte aligned):
 * kind 0 = silu, 1 = relu squared; fp32 math, bf16 results in the autocast rounding order.  plm_act_bwd: du = dout * act'(u). */
int plm_act_fwd(const uint16_t* u, uint16_t* out, int64_t n, int kind, void* stream);
int plm_act_bwd(const uint16_t* dout, const uint16_t* u, uint16_t* du, int64_t n, int kind, void* stream);

/* ---- bf16 MFMA GEMMs (nn.Linear: transformer.py:36-37,42,67,97,114; components.py:50-51)
 * nt: C[M,N] = alpha * A[M,K] · B[N,K]^T        A,B bf16 K-contiguous (y = x W^T, and dX = dY (W^T)^T)
 * tn: C[M,N] (+)= alpha * A[K,M]^T · B[K,N]     A,B bf16, contraction over rows (dW = dY^T X), C fp32
 * c_dtype: 0 = bf16, 1 = fp32.  accumulate (fp32 C only): C += result.
 * alpha_dev: optional device pointer to one fp32 scale (NULL = 1).
 * Requirements: K % 8 == 0 (nt) ; M % 8 == 0 and N % 8 == 0 (tn); ld* % 8 == 0; 16-byte aligned bases.
 * tn splits the contraction over `splits` slabs when M*N is too small to fill the chip; it needs a
 * fp32 workspace of plm_gemm_tn_workspace_bytes(M,N,K) bytes (0 when no split is used). */
int plm_gemm_bf16_nt(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, void* C, int64_t ldc,
                     int64_t M, int64_t N, int64_t K, int c_dtype, int accumulate, const float* alpha_dev, void* stream);
/* same as plm_gemm_bf16_nt with an explicit kernel choice (autotuning / A-B measurements / tests):
 * variant 0 = automatic, 1 = 128x128 register-staged, 2 = 128x128 LDS-DMA double-buffered,
 * 4 / 5 / 6 / 7 = persistent 256x256 / 256x192 / 256x128 / 128x192 with the deep-prefetch ring (half-tile slots refilled two
 *             K-tiles ahead) and offset wave groups - the kernels the automatic policy chooses from (128x192, round 5: the short
 *             batches, M = 8192 of config_doc_mask.yaml:35); 3 = 4 (kept for callers of round 1)
 * (3..7: bf16 C, no accumulate; 2..7: K % 64 == 0, N % 8 == 0, ldc % 8 == 0). */
int plm_gemm_bf16_nt_ex(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, void* C, int64_t ldc,
                        int64_t M, int64_t N, int64_t K, int c_dtype, int accumulate, const float* alpha_dev, int variant,
                        void* stream);
/* nt with an optional caller-owned fp32 workspace (plm_gemm_nt_workspace_bytes; 0 = none needed): with it the automatic
 * choice may use the hybrid whole-K + split-K schedule on 256x256 tiles, which removes the round quantisation of shapes
 * such as N = 768 (384 tiles on 256 CUs).  Without a workspace the call behaves exactly like plm_gemm_bf16_nt_ex. */
size_t plm_gemm_nt_workspace_bytes(int64_t M, int64_t N, int64_t K);
int plm_gemm_bf16_nt_ws(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, void* C, int64_t ldc,
                        int64_t M, int64_t N, int64_t K, int c_dtype, int accumulate, const float* alpha_dev, int variant,
                        void* workspace, size_t workspace_bytes, void* stream);
size_t plm_gemm_tn_workspace_bytes(int64_t M, int64_t N, int64_t K);
/* Several tn problems with the SAME contraction length K (the dW GEMMs of one or more transformer blocks: engine/engine.py's
 * backward reaches them one after the other, none of them has a consumer inside backward) as ONE launch over the union of
 * their 256x256 output tiles - whole-K tiles written directly for the full rounds of the persistent grid, split-K + one
 * reduce for the remaining tiles: C_p[M_p, N_p] (+)= alpha_p * A_p[K, M_p]^T B_p[K, N_p].  count <= 48; row strides < 2^31;
 * workspace from the query below (0 = shapes cannot be grouped). */
typedef struct plm_tn_problem {
  const uint16_t* A; int64_t lda;
  const uint16_t* B; int64_t ldb;
  float* C; int64_t ldc;
  int64_t M, N;
  int accumulate;
  const float* alpha_dev;
} plm_tn_problem;
size_t plm_gemm_tn_grouped_workspace_bytes(const int64_t* Ms, const int64_t* Ns, int count, int64_t K);
int plm_gemm_bf16_tn_grouped(const plm_tn_problem* probs, int count, int64_t K, void* workspace, size_t workspace_bytes,
                             void* stream);
int plm_gemm_bf16_tn(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, float* C, int64_t ldc,
                     int64_t M, int64_t N, int64_t K, int accumulate, const float* alpha_dev,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- RoPE + causal / document-masked attention
 * (models/transformer.py:43-65, models/embeddings.py:15-30, data/datasets/data_prep_utils.py:7-23)
 * qkv bf16[B*T, 3*nh*hd] straight from w_qkv (q | k | v column blocks, head h = cols h*hd..), T % 4 == 0; hd == 64 takes the tuned kernels
 * described below (every shipped config), hd == 32 or 128 (models/transformer.py:34 allows any dim // n_heads) a plain kernel family
 * (csrc/attn_generic.hip: element-wise masks, no plan needed, the inverse rotation as a separate in-place pass) behind the same entry points.
 * rope_cos/sin fp32[T, hd/2] (interleaved-pair convention).  doc_start int32[B,T] or NULL (pure causal):
 * query i attends key j iff doc_start[i] <= j <= i (doc_start non-decreasing in i).
 * plm_rope_qk : rotates the q and k blocks of qkv IN PLACE (fp32 math, bf16 result).  The training step does not launch it: the
 *               rotation is fused into plm_qkv_rope_bf16's GEMM epilogue; this is that entry point's fallback and the tests' yardstick.
 * Two kernel families behind the same two entry points: doc_start == NULL (plain causal batches) takes the 256-query-tile kernels of
 * csrc/attn_causal.hip, a document mask the 128-row-tile kernels of csrc/attn_doc.hip (+ the DOC mode of the causal dK/dV kernel); lse / delta are only meaningful within one
 * forward / backward pair of the same family (pass the same doc_start to both).
 * plm_attn_fwd: qkv with q,k ALREADY rotated -> out bf16[B*T, nh*hd], lse fp32[B, nh, T] (BASE-2 log-sum-exp of the
 *               scaled scores, = LSE / ln 2: the form plm_attn_bwd's exp2 consumes; opaque to the caller otherwise).  No transposed / contiguous copies of q, k, v are made anywhere.
 * plm_attn_bwd: same rotated qkv; dqkv bf16[B*T, 3*nh*hd] = gradient w.r.t. the PRE-rotation q, k (the inverse
 *               rotation is applied in the kernels' epilogues) and v; delta fp32[B,nh,T] scratch (+-rowsum(dO * O), written by the dQ
 *               kernel and read by the dK/dV kernel that follows it; stored negated: opaque to the caller).
 * qkv, out, dout, dqkv and the RoPE tables must be 16-byte aligned (LDS-DMA sources, whole-row 16-byte epilogue stores); misaligned
 * pointers are refused with PLM_E_INVALID. */
int plm_rope_qk(uint16_t* qkv, const float* rope_cos, const float* rope_sin, int64_t B, int64_t T, int64_t nh, int64_t hd,
                void* stream);
/* w_qkv projection + RoPE (transformer.py:42-47): QKV[M, 3*nh*hd] = X[M,K] W[3*nh*hd, K]^T with the q | k column blocks rotated
 * (ldq must be 3*nh*hd).  Default path: ONE launch - the rotation happens on the store side of the GEMM's epilogue (the bf16 values
 * the GEMM would have written are rotated on their way from the epilogue's LDS transposition scratch to memory; K % 64 == 0,
 * M >= 512, 16-byte aligned operands).  Other shapes, and PLM_GEMM_V1, take the fallback: the plain GEMM followed by the in-place
 * plm_rope_qk pass.  Both paths produce the same bits. */
int plm_qkv_rope_bf16(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, uint16_t* QKV, int64_t ldq, int64_t M,
                      int64_t K, const float* rope_cos, const float* rope_sin, int64_t B, int64_t T, int64_t nh, int64_t hd,
                      void* stream);
/* fc1 of the SwiGLU MLP with the activation in the GEMM epilogue (models/components.py:50-56):
 * U[M, 2h] = X[M,K] W[2h,K]^T (gate | up columns, dense, kept for backward) and ACT[M, h] = bf16(bf16(silu(gate)) * up), the
 * reference's autocast rounding order.  One launch when 2h % 256 == 0, K % 64 == 0, M >= 512; otherwise GEMM + plm_swiglu_fwd
 * (same bits). */
int plm_fc1_swiglu_bf16(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, uint16_t* U, uint16_t* ACT, int64_t M,
                        int64_t h, int64_t K, void* stream);
/* dX of fc2 with the SwiGLU backward in the GEMM epilogue: DU[M, 2h] = swiglu_bwd(dY[M,K] W2T[h,K]^T, U[M,2h]) where W2T is the
 * transposed bf16 copy of fc2's weight and U the saved fc1 output; d(act) is never stored.  One launch when h % 256 == 0,
 * K % 64 == 0, M >= 512; otherwise GEMM + plm_swiglu_bwd through `scratch` (M*h bf16).  With scratch == NULL the call either takes the
 * one-launch path or returns PLM_E_WORKSPACE without launching anything. */
int plm_fc2_dx_swiglu_bwd_bf16(const uint16_t* dY, int64_t lddy, const uint16_t* W2T, int64_t ldw, const uint16_t* U, uint16_t* DU,
                               uint16_t* scratch, int64_t M, int64_t h, int64_t K, void* stream);
/* Document masks (models/transformer.py:52-61 with the masks of data/datasets/data_prep_utils.py:7-23, stacked at engine/engine.py:21-23): a batch's
 * doc_start[B,T] comes with a PLAN, built once per batch by plm_attn_doc_plan and shared by every layer's forward and backward launches:
 * doc_end[B,T] (the first query that no longer sees a key: the dK/dV kernel's mask becomes two thresholds per key) and the batch's 128-row
 * query / key tiles sorted by the number of 64-row tiles they actually walk, heaviest first - the launch order of the kernels; when the
 * grid of B * ceil(T/128) * nh workgroups is resident at once, the heaviest tiles enter the lists as two 64-row halves (half the chain each).
 * plan is caller-owned device memory of plm_attn_doc_plan_bytes(B, T) bytes, 16-byte aligned; doc_start must be non-decreasing along T with
 * doc_start[b][i] <= i.  plm_attn_fwd / plm_attn_bwd: doc_start == NULL -> causal (doc_plan ignored); otherwise doc_plan is required
 * (PLM_E_INVALID without it). */
/* The reference's own mask format -> doc_start: mask is the bool [B, T, T] tensor of engine/engine.py:21-23 (one byte per element, nonzero =
 * may attend), doc_start[b][i] = first allowed key of row i.  Every row is checked to be exactly [doc_start, i] (the block-diagonal causal
 * masks of data_prep_utils.py:7-23 are); status[0] (caller-zeroed int32) is set to 1 when some row is not - such a mask cannot be expressed
 * as doc_start and the caller must refuse it. */
int plm_attn_doc_start_from_mask(const uint8_t* mask, int32_t* doc_start, int32_t* status, int64_t B, int64_t T, void* stream);
int64_t plm_attn_doc_plan_bytes(int64_t B, int64_t T);
int plm_attn_doc_plan(const int32_t* doc_start, int32_t* plan, int64_t B, int64_t T, int64_t nh, void* stream);
int plm_attn_fwd(const uint16_t* qkv, const int32_t* doc_start, const int32_t* doc_plan, uint16_t* out, float* lse, int64_t B, int64_t T,
                 int64_t nh, int64_t hd, void* stream);
int plm_attn_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse,
                 const float* rope_cos, const float* rope_sin, const int32_t* doc_start, const int32_t* doc_plan,
                 uint16_t* dqkv, float* delta, int64_t B, int64_t T, int64_t nh, int64_t hd, void* stream);

/* Dense boolean masks (models/transformer.py:52-61 hands ANY bool [B,T,T] mask to SDPA: sliding windows, prefix-LM, padding, random
 * patterns; keys after the query included).  A third mask mode with its own kernels (csrc/attn_masked.hip, head dims 32, 64, 128, T % 4 == 0).
 * plm_attn_mask_pack: mask bool [M, T, T] (one byte per element, nonzero = may attend; the reference's layout) -> bits uint64 [M, T, ceil(T/64)]
 *   (bit j % 64 of word (m, i, j / 64) = mask[m, i, j]; bits past T are 0) and tile_class uint8 [M, ceil(T/128), ceil(T/64)] of the 128-query x
 *   64-key tiles the kernels walk (0: no bit set - skipped; 1: every in-range bit set - the unmasked path; 2: mixed).  batch_stride 1: M = B,
 *   mask m is sequence m's; batch_stride 0: M = 1, one [T, T] mask shared by every sequence (packed once).  One launch, deterministic.
 *   plm_attn_mask_bytes(M, T): bytes of bits followed by tile_class (the bits take M*T*ceil(T/64)*8 bytes, a multiple of 16; tile_class starts
 *   there); the caller owns the storage.
 * plm_attn_fwd_masked / plm_attn_bwd_masked: the plm_attn_fwd / plm_attn_bwd contract (rotated qkv, base-2 lse, dqkv w.r.t. the UN-rotated
 *   q, k) under the packed mask, with the same batch_stride as the pack.  delta is stored with the plain sign (+rowsum(dO * O)) for every head dim.
 *   A query row with no allowed key follows torch's SDPA: out = 0, lse = +INFINITY (the backward's exp2(s c - lse) is then exactly 0), and the
 *   row's dQ and its contributions to dK / dV are 0.  Deterministic (no atomics).
 * NULL pointers, hd not in {32, 64, 128}, a bad shape or batch_stride, and qkv / out / dout / dqkv / RoPE tables / bits / tile_class that are not
 * 16-byte aligned are refused with PLM_E_INVALID before anything is launched. */
int64_t plm_attn_mask_bytes(int64_t B, int64_t T);
int plm_attn_mask_pack(const uint8_t* mask, int64_t batch_stride, uint64_t* bits, uint8_t* tile_class, int64_t B, int64_t T, void* stream);
int plm_attn_fwd_masked(const uint16_t* qkv, const uint64_t* bits, const uint8_t* tile_class, int64_t batch_stride, uint16_t* out, float* lse,
                        int64_t B, int64_t T, int64_t nh, int64_t hd, void* stream);
int plm_attn_bwd_masked(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse, const float* rope_cos,
                        const float* rope_sin, const uint64_t* bits, const uint8_t* tile_class, int64_t batch_stride, uint16_t* dqkv,
                        float* delta, int64_t B, int64_t T, int64_t nh, int64_t hd, void* stream);

/* ---- KV-cached generation -----
 * Every argument check of these entry points comes before any HIP call.
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

/* ---- cache extension: a chunk of up to n tokens per sequence on top of a live cache -----
 * Every argument check of these entry points comes before any HIP call.  The cache is the one above.  A chunk is n rows per sequence,
 * row b*n + r = chunk row r of sequence b; lens0 int32[B] is the cache length before the chunk; n_new int32[B] is the number of real rows
 * of every sequence's chunk, c_b = n_new[b] clamped to [0, n] - or NULL: c_b = n for every sequence.
 *
 * plm_kv_append_rope_rows: qkv bf16 [B*n, ld_qkv] is the UN-rotated projection.  For rows r < c_b: q and k are rotated at position
 * lens0[b] + r with the arithmetic of plm_rope_qk (same bits), rotated q goes to q_out bf16 [B*n, nh*hd] row b*n + r, rotated k and the
 * untouched v to kv[b, lens0[b] + r, 0 : 2*nh*hd].  Rows r >= c_b write no cache row and a q_out row of zeros: every byte of q_out is
 * defined.  A sequence with lens0[b] < 0 or lens0[b] + c_b > min(Tmax, rope_T) is refused on the device: none of its cache rows is
 * written, its q_out rows are zeros and the caller-zeroed status[0] is set to 1; the other sequences are unaffected.  One launch.
 * PLM_E_INVALID before anything is launched: NULL pointers (n_new excepted), a head_dim other than 32 / 64 / 128, n < 1 or B*n >= 2^31,
 * a bad shape, row strides that are not multiples of 8 or shorter than a row, qkv / q_out / kv / tables not 16-byte aligned.
 *
 * plm_attn_extend: q bf16 [B*n, nh*hd], already rotated (q_out above).  lens0 is clamped to [0, Tmax].  Query (b, r) with r < c_b attends
 * keys 0 .. min(lens0[b] + r, Tmax - 1) inclusive - its own key, just appended, included.  Writes out bf16 [B*n, nh*hd] and, unless NULL,
 * lse fp32 [B, nh, n]: the base-2 log-sum-exp of the scaled scores (plm_attn_fwd's convention), comparable with row lens0[b] + r of a full
 * causal forward.  Rows r >= c_b give out = 0 and lse = +INFINITY.  Cache rows at and beyond lens0[b] + c_b are never loaded (they may
 * hold anything, NaN included); q rows r >= c_b are never loaded either.
 * The keys 0 .. lens0[b] + c_b - 1 of sequence b are cut into S contiguous ranges as plm_attn_decode cuts them; a
 * (B*nh*ceil(n/128)) x S grid of MFMA workgroups (128 query rows x 64-key tiles) leaves fp32 partials (max, sum, acc[hd]) per (query row,
 * split) in the workspace, and a second launch combines them in split order, skipping empty ones.  S = 1 writes out directly: one launch.
 * No atomics: bit-reproducible, and for a forced S independent of the other sequences of the batch.  splits: 0 = automatic (a function of
 * B, n, nh, Tmax and the CU count only - nothing is read back), 1..64 forced.  workspace: plm_attn_extend_workspace_bytes(B, n, nh, hd,
 * Tmax, splits) bytes for the same splits argument, 16-byte aligned, caller-owned (the query returns 0 for arguments the launch refuses).
 * NULL pointers (lse and n_new excepted), a head_dim other than 32 / 64 / 128, n < 1, B*n >= 2^31, bases that are not 16-byte aligned,
 * splits outside 0..64 give PLM_E_INVALID and a short workspace PLM_E_WORKSPACE before anything is launched. */
int plm_kv_append_rope_rows(const uint16_t* qkv, int64_t ld_qkv, const int32_t* lens0, const int32_t* n_new, const float* rope_cos,
                            const float* rope_sin, int64_t rope_T, uint16_t* q_out, uint16_t* kv, int64_t ld_kv, int32_t* status, int64_t B,
                            int64_t n, int64_t Tmax, int64_t nh, int64_t hd, void* stream);
size_t plm_attn_extend_workspace_bytes(int64_t B, int64_t n, int64_t nh, int64_t hd, int64_t Tmax, int splits);
int plm_attn_extend(const uint16_t* q, const uint16_t* kv, int64_t ld_kv, const int32_t* lens0, const int32_t* n_new, uint16_t* out,
                    float* lse, int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd, int splits, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- the fused decode step: skinny-M layer kernels and one call per layer -----
 * Every argument check of these entry points comes before any HIP call; none falls back to another path.
 * M = B rows, one decode token per sequence, 1 <= M <= 32.  Weights are the bf16 shadows [N, K], contiguous (the layout plm_gemm_bf16_nt
 * consumes), read once per launch; accumulation is fp32; the K split across the four waves of a workgroup is added in wave order (no
 * atomics: two runs are bit-equal).  Every rounding point of the unfused step is kept; only the order of the fp32 sums differs.
 *
 * plm_decode_norm_qkv_append_bf16 (replaces plm_rmsnorm_fwd + plm_gemm_bf16_nt + plm_kv_append_rope): x fp32 [B, d], d = nh*hd;
 * n = bf16(x * rstd * norm_w) with plm_rmsnorm_fwd's rounding; qkv = bf16(n w_qkv^T), w_qkv bf16 [3d, d]; the q and k columns are rotated
 * at position pos[b] with plm_kv_append_rope's arithmetic on the bf16 values; rotated q goes to q_out bf16 [B, d], rotated k | v to
 * kv[b, pos[b], 0 : 2d] of the cache kv[B, Tmax, ld_kv] above.  A pos[b] outside [0, min(Tmax, rope_T)) stores nothing for that sequence,
 * writes a q_out row of zeros and sets the caller-zeroed status[0] to 1.  One launch.
 *
 * plm_decode_gemm_residual_bf16 (replaces plm_gemm_bf16_nt and the residual add of the next norm): x[M, N] += float(bf16(A W^T)) in place
 * on the fp32 stream; A bf16 [M, K], W bf16 [N, K].  One launch.
 *
 * plm_decode_norm_fc1_act_bf16 (replaces plm_rmsnorm_fwd + plm_gemm_bf16_nt + plm_swiglu_fwd / plm_act_fwd): the norm as above, u =
 * bf16(n w_fc1^T), then on the bf16 values act bf16 [M, hidden] = PLM_DECODE_MLP_GLU: plm_swiglu_fwd of u = gate | up, w_fc1 [2*hidden, d];
 * PLM_DECODE_MLP_SILU / PLM_DECODE_MLP_RELU_SQ: plm_act_fwd kind 0 / 1, w_fc1 [hidden, d].  One launch.
 *
 * plm_decode_layer_bf16: a whole decode layer on `stream` from one call - the qkv stage, plm_attn_decode's two launches (lens, splits as
 * there), the residual stage with w_out [d, d], the fc1 stage, the residual stage with w_fc2 [d, hidden]: six launches.  x fp32 [B, d] is
 * updated in place.  q, the attention output, the activation and plm_attn_decode's partials live in the workspace:
 * plm_decode_layer_workspace_bytes(B, nh, hd, hidden, Tmax, splits) bytes for the same splits argument, 16-byte aligned, caller-owned; the
 * query is a function of its arguments alone and returns 0 for arguments the launch refuses.
 *
 * PLM_E_INVALID before anything is launched: NULL pointers, M (B) outside 1..32, a head_dim other than 32 / 64 / 128, d % 32 != 0,
 * hidden % 32 != 0, N % 16 != 0 or K % 32 != 0, an unknown mlp_kind, a cache row stride that is no multiple of 8 or shorter than 2d, splits
 * outside 0..64, x / norm weights / weights / q_out / kv / A / act / workspace not 16-byte aligned; a short workspace gives
 * PLM_E_WORKSPACE. */
#define PLM_DECODE_MLP_GLU 0
#define PLM_DECODE_MLP_SILU 1
#define PLM_DECODE_MLP_RELU_SQ 2
int plm_decode_norm_qkv_append_bf16(const float* x, const float* norm_w, float eps, const uint16_t* w_qkv, const int32_t* pos,
                                    const float* rope_cos, const float* rope_sin, int64_t rope_T, uint16_t* q_out, uint16_t* kv, int64_t ld_kv,
                                    int32_t* status, int64_t B, int64_t Tmax, int64_t nh, int64_t hd, void* stream);
int plm_decode_gemm_residual_bf16(float* x, const uint16_t* A, const uint16_t* W, int64_t M, int64_t N, int64_t K, void* stream);
int plm_decode_norm_fc1_act_bf16(const float* x, const float* norm_w, float eps, const uint16_t* w_fc1, uint16_t* act, int64_t M, int64_t d,
                                 int64_t hidden, int mlp_kind, void* stream);
size_t plm_decode_layer_workspace_bytes(int64_t B, int64_t nh, int64_t hd, int64_t hidden, int64_t Tmax, int splits);
int plm_decode_layer_bf16(float* x, const float* attn_norm_w, const float* mlp_norm_w, float eps, const uint16_t* w_qkv, const uint16_t* w_out,
                          const uint16_t* w_fc1, const uint16_t* w_fc2, const int32_t* pos, const int32_t* lens, const float* rope_cos,
                          const float* rope_sin, int64_t rope_T, uint16_t* kv, int64_t ld_kv, int32_t* status, int64_t B, int64_t Tmax,
                          int64_t nh, int64_t hd, int64_t hidden, int mlp_kind, int splits, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- the fused extend: chunk rows on the skinny-M layer kernels -----
 * Every argument check of these entry points comes before any HIP call; none falls back to another path.  A chunk is n rows per sequence,
 * row b*n + r = chunk row r of sequence b, M = B*n rows with 1 <= B*n <= 32; lens0 int32[B], n_new int32[B] or NULL and c_b are those of
 * the cache extension above.  plm_decode_gemm_residual_bf16 and plm_decode_norm_fc1_act_bf16 serve chunk rows as they are (they never
 * look at positions).
 *
 * plm_extend_norm_qkv_append_bf16 (replaces plm_rmsnorm_fwd + plm_gemm_bf16_nt + plm_kv_append_rope_rows): x fp32 [B*n, d]; the norm, the
 * GEMM and the rounding points of plm_decode_norm_qkv_append_bf16 (the same core: a full chunk gives the bits that entry point gives for
 * the same rows at pos = lens0[b] + r), then plm_kv_append_rope_rows's contract on the bf16 values.  Rows r < c_b of a sequence that
 * fits: q and k rotated at position lens0[b] + r, rotated q to q_out bf16 [B*n, d] row b*n + r, rotated k | v to kv[b, lens0[b] + r,
 * 0 : 2d].  Rows r >= c_b write no cache row and a q_out row of zeros.  A sequence with lens0[b] < 0 or lens0[b] + c_b > min(Tmax, rope_T)
 * is refused on the device: none of its cache rows is written, its n q_out rows are zeros and the caller-zeroed status[0] is set to 1; the
 * other sequences are unaffected.  Every byte of q_out is defined.  One launch.
 *
 * plm_extend_layer_bf16: a whole layer over a chunk on `stream` from one call - the qkv stage above, plm_attn_extend's two launches (one
 * when it resolves to a single split; lens0, n_new, splits as there), the residual stage with w_out [d, d], the fc1 stage, the residual
 * stage with w_fc2 [d, hidden]: at most six launches.  x fp32 [B*n, d] is updated in place (padding rows too: they hold finite values
 * that mean nothing).  q, the attention output, the activation and plm_attn_extend's partials live in the workspace:
 * plm_extend_layer_workspace_bytes(B, n, nh, hd, hidden, Tmax, splits) bytes for the same splits argument, 16-byte aligned, caller-owned;
 * the query is a function of its arguments alone and returns 0 for arguments the launch refuses.
 *
 * PLM_E_INVALID before anything is launched: what the fused decode step refuses, with B*n in place of M; NULL pointers (n_new
 * excepted), n < 1, B*n outside 1..32; a short workspace gives PLM_E_WORKSPACE. */
int plm_extend_norm_qkv_append_bf16(const float* x, const float* norm_w, float eps, const uint16_t* w_qkv, const int32_t* lens0,
                                    const int32_t* n_new, const float* rope_cos, const float* rope_sin, int64_t rope_T, uint16_t* q_out,
                                    uint16_t* kv, int64_t ld_kv, int32_t* status, int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd,
                                    void* stream);
size_t plm_extend_layer_workspace_bytes(int64_t B, int64_t n, int64_t nh, int64_t hd, int64_t hidden, int64_t Tmax, int splits);
int plm_extend_layer_bf16(float* x, const float* attn_norm_w, const float* mlp_norm_w, float eps, const uint16_t* w_qkv, const uint16_t* w_out,
                          const uint16_t* w_fc1, const uint16_t* w_fc2, const int32_t* lens0, const int32_t* n_new, const float* rope_cos,
                          const float* rope_sin, int64_t rope_T, uint16_t* kv, int64_t ld_kv, int32_t* status, int64_t B, int64_t n,
                          int64_t Tmax, int64_t nh, int64_t hd, int64_t hidden, int mlp_kind, int splits, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- the FP8 KV cache: block-scaled e4m3 rows for decode, extend and the fused layers -----
 * Every argument check of these entry points comes before any HIP call.  An alternative to the bf16 cache above, chosen per cache; the
 * entry points above are untouched.  head_dim is 32, 64 or 128, dm = nh*hd.
 *
 * Cache layout: one uint8 buffer per layer, kv8[B, Tmax, ld_kv8] with ld_kv8 in BYTES, a multiple of 16 and at least 2*dm + dm/8;
 * sequence b starts at b * Tmax * ld_kv8.  Row (b, j) = [ k codes dm | v codes dm | k scales dm/16 | v scales dm/16 ]: OCP e4m3fn codes
 * (not fnuz) and one E8M0 scale byte per 16 consecutive elements of a head.  Quantisation is of the bf16 values the bf16 cache would
 * hold (k after RoPE), block by block: e = the smallest exponent with amax <= 448 * 2^e, clamped to [-127, 127]; scale byte e + 127; code
 * = RNE-e4m3fn(x * 2^-e) with subnormals; amax = 0 gives scale byte 0 and zero codes; any non-finite value in the block gives scale byte
 * 0xFF and codes 0x7F.  Dequantisation is code * 2^(s - 127), NaN for s = 0xFF: exact in fp32 (the decode kernel) and in bf16 (the extend
 * kernel's LDS tile, plm_kv8_dequant_rows) unless the value lies below bf16's subnormal range (under 2^-133), where it rounds.  q, P,
 * the softmax statistics and the partials are never quantised.  Because dequantisation is exact, plm_attn_decode_kv8 /
 * plm_attn_extend_kv8 return, bit for bit, what plm_attn_decode / plm_attn_extend return on the plm_kv8_dequant_rows image of the cache.
 *
 * plm_kv8_quant_rows: src bf16 [B, T, ld_src] (k | v rows, 2*dm columns used; ld_src >= 2*dm, a multiple of 8) is quantised into cache
 * rows 0 .. T-1 of every sequence (a prefill's write).  plm_kv8_dequant_rows: cache rows 0 .. T-1 of every sequence to dst bf16
 * [B, T, ld_dst].  One launch each.  PLM_E_INVALID before anything is launched: NULL pointers, a head_dim other than 32 / 64 / 128,
 * T < 1 or T > Tmax, B*T >= 2^31, a bf16 stride that is no multiple of 8 or shorter than 2*dm, an ld_kv8 that is no multiple of 16 or
 * shorter than 2*dm + dm/8, bases that are not 16-byte aligned.
 *
 * plm_kv8_append_rope_rows: plm_kv_append_rope_rows's contract (lens0, n_new, c_b, the refusal on the device with status[0] = 1, zeroed
 * q_out rows for rows without a cache row, the same rotation and the same q_out bits) with the rotated k | v quantised into kv8[b,
 * lens0[b] + r].  A decode step is its n = 1 case (lens0 = the positions, n_new = NULL).  One launch.  Its refusals are
 * plm_kv_append_rope_rows's, with the ld_kv8 rule above for the cache stride.
 *
 * plm_attn_decode_kv8 / plm_attn_extend_kv8: plm_attn_decode / plm_attn_extend over this cache.  Same arguments otherwise, same split
 * rule, partial layout, combine launch and workspace (plm_attn_decode_workspace_bytes / plm_attn_extend_workspace_bytes), same refusals
 * with the ld_kv8 rule above (PLM_E_INVALID; a short workspace PLM_E_WORKSPACE).  Rows at and beyond the valid length are never loaded.
 *
 * plm_extend_norm_qkv_append_kv8_bf16, plm_decode_layer_kv8_bf16, plm_extend_layer_kv8_bf16: the fused qkv stage and the two layer
 * calls of the sections above over this cache (the decode qkv stage is the extend stage at n = 1, n_new = NULL).  The stage rounds to
 * bf16 and rotates as plm_extend_norm_qkv_append_bf16 does, then quantises: q_out and the quantised values are that entry point's bits.
 * The layers take plm_decode_layer_workspace_bytes / plm_extend_layer_workspace_bytes bytes.  Their refusals are those entry points',
 * with the ld_kv8 rule above, all before the first launch. */
int plm_kv8_quant_rows(const uint16_t* src, int64_t ld_src, uint8_t* kv8, int64_t ld_kv8, int64_t B, int64_t T, int64_t Tmax, int64_t nh,
                       int64_t hd, void* stream);
int plm_kv8_dequant_rows(const uint8_t* kv8, int64_t ld_kv8, uint16_t* dst, int64_t ld_dst, int64_t B, int64_t T, int64_t Tmax, int64_t nh,
                         int64_t hd, void* stream);
int plm_kv8_append_rope_rows(const uint16_t* qkv, int64_t ld_qkv, const int32_t* lens0, const int32_t* n_new, const float* rope_cos,
                             const float* rope_sin, int64_t rope_T, uint16_t* q_out, uint8_t* kv8, int64_t ld_kv8, int32_t* status, int64_t B,
                             int64_t n, int64_t Tmax, int64_t nh, int64_t hd, void* stream);
int plm_attn_decode_kv8(const uint16_t* q, const uint8_t* kv8, int64_t ld_kv8, const int32_t* lens, uint16_t* out, float* lse, int64_t B,
                        int64_t Tmax, int64_t nh, int64_t hd, int splits, void* workspace, size_t workspace_bytes, void* stream);
int plm_attn_extend_kv8(const uint16_t* q, const uint8_t* kv8, int64_t ld_kv8, const int32_t* lens0, const int32_t* n_new, uint16_t* out,
                        float* lse, int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd, int splits, void* workspace,
                        size_t workspace_bytes, void* stream);
int plm_extend_norm_qkv_append_kv8_bf16(const float* x, const float* norm_w, float eps, const uint16_t* w_qkv, const int32_t* lens0,
                                        const int32_t* n_new, const float* rope_cos, const float* rope_sin, int64_t rope_T, uint16_t* q_out,
                                        uint8_t* kv8, int64_t ld_kv8, int32_t* status, int64_t B, int64_t n, int64_t Tmax, int64_t nh,
                                        int64_t hd, void* stream);
int plm_decode_layer_kv8_bf16(float* x, const float* attn_norm_w, const float* mlp_norm_w, float eps, const uint16_t* w_qkv,
                              const uint16_t* w_out, const uint16_t* w_fc1, const uint16_t* w_fc2, const int32_t* pos, const int32_t* lens,
                              const float* rope_cos, const float* rope_sin, int64_t rope_T, uint8_t* kv8, int64_t ld_kv8, int32_t* status,
                              int64_t B, int64_t Tmax, int64_t nh, int64_t hd, int64_t hidden, int mlp_kind, int splits, void* workspace,
                              size_t workspace_bytes, void* stream);
int plm_extend_layer_kv8_bf16(float* x, const float* attn_norm_w, const float* mlp_norm_w, float eps, const uint16_t* w_qkv,
                              const uint16_t* w_out, const uint16_t* w_fc1, const uint16_t* w_fc2, const int32_t* lens0, const int32_t* n_new,
                              const float* rope_cos, const float* rope_sin, int64_t rope_T, uint8_t* kv8, int64_t ld_kv8, int32_t* status,
                              int64_t B, int64_t n, int64_t Tmax, int64_t nh, int64_t hd, int64_t hidden, int mlp_kind, int splits,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- temperature / top-k / top-p sampling of one token per row -----
 * Every argument check comes before any HIP call.
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

/* ---- speculative-sampling acceptance of k drafted tokens per sequence -----
 * Every argument check comes before any HIP call.
 * p_logits bf16 [B*(k+1), ldp]: the target's chunk rows, row b*(k+1) + r (what extend(all_rows, logits) returns); q_logits bf16
 * [k*B, ldq]: the draft's rows, step-major, row r*B + b.  Any 2-byte aligned bases and any ld >= V: columns >= V are never loaded.
 * draft_tok int64 [k, B]: the token the draft drew at step r.  p_cutoff fp32 [B*(k+1)] and q_cutoff fp32 [k*B]: the `cutoff` output of
 * plm_sample_logits_bf16 on those rows at this temperature - a row's distribution is that sampler's: weight exp((x - x_max) /
 * temperature) on {i : x_i finite and x_i >= cutoff}, 0 elsewhere (a NaN cutoff keeps nothing), with the sampler's own fixed-point
 * weights.  p_tok int64 [B*(k+1)]: that sampler's token of every target row.  u_accept fp32 [k, B] and u_resid fp32 [B]: uniforms, clamped
 * on the device as the sampler clamps u.
 *
 * The rule, per sequence b.  For r = 0 .. k-1 in order, with x = draft_tok[r, b]: alpha = min(1, p_r(x) / q_r(x)); alpha = 0 when x is
 * outside [0, V) or p_r(x) = 0 (outside p's kept set), alpha = 1 when q_r(x) = 0 < p_r(x); row r is accepted while u_accept[r, b] < alpha.
 * n_accept counts the accepted rows.  n_accept = k: next_tok = p_tok of row k (the bonus token).  Else, at the first rejected row a,
 * next_tok = the lowest i with C_i > u_resid[b] * R, C the running sum in ascending column order of max(0, p_a(i) - q_a(i)) and R its
 * total; R = 0 (or a row without a finite logit): next_tok = p_tok of row a.
 * Outputs: n_accept int32 [B] in [0, k]; next_tok int64 [B], always in [0, V); logp fp32 [B, k+1]: entry j <= n_accept is
 * log softmax over all V raw logits of target row j at temperature 1 (as plm_sample_logits_bf16 states it) of the token emitted there -
 * draft_tok[j, b], or next_tok at j = n_accept - and 0 beyond.
 * Two launches (one workgroup per drafted row, then one per sequence; logp carries the verdicts between them), no workspace, nothing read
 * back.  Sequence b's outputs depend on sequence b's inputs alone, and the same inputs give the same bits on every run (64-bit
 * fixed-point sums; the quotients are fp64 expressions of those integers).
 * PLM_E_INVALID before anything is launched for: a NULL pointer, B < 1 or B >= 2^26, k < 1 or k > 31, V < 1 or V >= 2^31, ldp < V or
 * ldq < V, a logits base that is not 2-byte aligned, a temperature that is not finite or <= 0. */
int plm_spec_verify_bf16(const uint16_t* p_logits, int64_t ldp, const uint16_t* q_logits, int64_t ldq, const int64_t* draft_tok,
                         const float* p_cutoff, const float* q_cutoff, const int64_t* p_tok, const float* u_accept, const float* u_resid,
                         float temperature, int32_t* n_accept, int64_t* next_tok, float* logp, int64_t B, int64_t k, int64_t V,
                         void* stream);

/* ---- draft-free speculative decoding: n-gram lookup drafts and their one-hot acceptance -----
 * Every argument check of these entry points comes before any HIP call.
 *
 * plm_lookup_draft_i64: a sequence proposes the tokens that followed the most recent earlier occurrence of its own last few tokens.
 * hist int64 [B, ld] (in/out): every sequence's token history, lens int32 [B] (in/out) its length; add_tok int64 [B, ld_add] and n_add
 * int32 [B]: tokens to append first, c_b = n_add[b] clamped to [0, ld_add] of them (n_add NULL: c_b = ld_add; add_tok NULL: c_b = 0 and
 * n_add must be NULL too).  Integers only, one launch, one workgroup per sequence, no workspace, nothing read back; sequence b's outputs
 * depend on sequence b's inputs alone.
 *   append   add_tok[b, 0 : c_b] goes to hist[b, lens[b] : lens[b] + c_b] and lens[b] moves by c_b.  A sequence with lens[b] < 0 or
 *            lens[b] + c_b > ld is refused on the device: nothing of it is stored, lens[b] stays, n_prop[b] = match_len[b] = 0, its draft_tok
 *            row is zeros and the caller-zeroed status[0] is set to 1 (plm_kv_append_rope's convention); the others are unaffected.
 *   search   with L the new length: for every end e in [1, L-1], m(e) = the number of consecutive t = 1, 2, .. with hist[b, e-t] ==
 *            hist[b, L-t], counted up to min(g_max, e).  The candidates are the ends with m(e) >= g_min; the winner has the largest m and,
 *            among those, the largest e (the longest match, then the most recent one).
 *   propose  with a winner e and its period P = L - e: draft_tok[b, i] = hist[b, e + (i mod P)] for i < k (an overlapped copy: a loop
 *            shorter than k still yields k tokens), n_prop[b] = k, match_len[b] = m(e).  Without a candidate (always when L < 2):
 *            n_prop[b] = match_len[b] = 0 and the draft_tok row is zeros - a valid token id, so the padded chunk rows can be embedded.
 * Outputs: draft_tok int64 [B, k], n_prop int32 [B], match_len int32 [B] (may be NULL); every element is written.  hist beyond the new
 * length is neither read nor written.
 * PLM_E_INVALID before anything is launched for: a NULL pointer (add_tok, n_add, match_len excepted), n_add without add_tok, k < 1 or
 * k > 31, g_min < 1, g_min > g_max or g_max > 16, B < 1 or B >= 2^31, ld < 1 or ld >= 2^31, with add_tok ld_add < 1 or ld_add >= 2^31,
 * hist / add_tok / draft_tok not 8-byte aligned.
 *
 * plm_spec_verify_lookup_bf16: the acceptance rule of plm_spec_verify_bf16 for a deterministic draft (q one-hot on the proposed token).
 * p_logits bf16 [B*(k+1), ldp], row b*(k+1) + r, p_cutoff fp32 [B*(k+1)] and p_tok int64 [B*(k+1)] as plm_spec_verify_bf16 takes them
 * (plm_sample_logits_bf16 on those rows at this temperature); draft_tok int64 [B, k] (plm_lookup_draft_i64's layout); n_prop int32 [B]:
 * the rows of sequence b that hold a proposal - any value in [0, k] is honoured, others are clamped to it on the device; u_accept fp32
 * [k, B] and u_resid fp32 [B], clamped on the device as the sampler clamps u.
 * The rule, per sequence b.  For r = 0 .. n_prop[b]-1 in order, with x = draft_tok[b, r]: alpha = p_r(x), the sampler's own distribution -
 * its fixed-point weight w_x over the kept set's sum Z; alpha = 0 when x is outside [0, V), outside the kept set, or w_x rounds to 0.  Row
 * r is accepted while u_accept[r, b] < alpha, evaluated in integers as floor(u Z) < w_x.  a = the first rejected row, or n_prop[b] when
 * none is.  a = n_prop[b]: next_tok = p_tok of row a (the bonus token; with n_prop[b] = 0 the plain next token).  Else next_tok = the
 * lowest i with C_i > floor(u_resid[b] * R), C the running sum in ascending column order of row a's integer weights with column x's set
 * to 0 and R = Z - w_x its total; R = 0 (or a row without a finite logit): next_tok = p_tok of row a.
 * Outputs n_accept int32 [B] (= a, in [0, n_prop[b]]), next_tok int64 [B] in [0, V) and logp fp32 [B, k+1] with exactly the meanings
 * plm_spec_verify_bf16 states.  Two launches of its shape (logp carries the verdicts between them), no workspace, nothing read back;
 * every sum is a 64-bit integer and there is no quotient: bit-reproducible, sequence b's outputs depend on sequence b's inputs alone.
 * Rows at and beyond n_prop[b] of p_logits (row a itself excepted) and of draft_tok are never loaded.
 * PLM_E_INVALID before anything is launched for: a NULL pointer, B < 1 or B >= 2^26, k < 1 or k > 31, V < 1 or V >= 2^31, ldp < V, a
 * logits base that is not 2-byte aligned, a temperature that is not finite or <= 0. */
int plm_lookup_draft_i64(int64_t* hist, int64_t ld, int32_t* lens, const int64_t* add_tok, int64_t ld_add, const int32_t* n_add,
                         int64_t* draft_tok, int32_t* n_prop, int32_t* match_len, int32_t* status, int64_t B, int64_t k, int64_t g_min,
                         int64_t g_max, void* stream);
int plm_spec_verify_lookup_bf16(const uint16_t* p_logits, int64_t ldp, const int64_t* draft_tok, const int32_t* n_prop,
                                const float* p_cutoff, const int64_t* p_tok, const float* u_accept, const float* u_resid, float temperature,
                                int32_t* n_accept, int64_t* next_tok, float* logp, int64_t B, int64_t k, int64_t V, void* stream);

/* ---- fused cross-entropy forward+backward (engine/engine.py:81,111) -----
 * logits bf16[M, ld] (row stride ld >= V) are OVERWRITTEN with dlogits = (softmax - onehot) * grad_scale
 * (grad_scale = g/M); pad columns V..ld are set to zero so the buffer can feed a GEMM with K = ld.
 * loss_rows fp32[M] = logsumexp(l) - l[target].  Then plm_mean_f32 reduces to the scalar mean. */
int plm_ce_fwd_bwd(uint16_t* logits, const int64_t* targets, float* loss_rows, int64_t M, int64_t V, int64_t ld,
                   float grad_scale, void* stream);
int plm_mean_f32(const float* x, float* out, int64_t n, void* stream);

/* ---- forward-only scoring head -----
 * nll fp32[M] = logsumexp(l) - l[target] and lse fp32[M] = logsumexp(l) of the rows l = bf16(Y[M,K] W[V,K]^T) - the logits the
 * training head computes (plm_gemm_bf16_nt + plm_ce_fwd_bwd: same tile shape and K order, so the same bf16 values) - WITHOUT ever
 * storing them: the persistent NT kernel reduces every output tile to one (max, sum-exp) pair per row and a second launch combines
 * a row's pairs.  A target outside [0, V) is ignored: nll = 0 for that row, lse is written all the same.  lse may be NULL.
 * No gradient is produced.  workspace: plm_head_score_workspace_bytes(M, V, K) bytes (about M * ceil(V / 128) * 8), 16-byte
 * aligned, caller-owned.  NULL pointers, K % 64 != 0, row strides that are not multiples of 8, Y / W that are not 16-byte aligned
 * give PLM_E_INVALID and a short workspace PLM_E_WORKSPACE before anything is launched.  Shapes that plm_gemm_bf16_nt serves with
 * a 128x128 kernel (M < 512, V % 8 != 0) go through that kernel, 256 rows of logits at a time inside the workspace.
 * Deterministic (no atomics). */
size_t plm_head_score_workspace_bytes(int64_t M, int64_t V, int64_t K);
int plm_head_score_bf16(const uint16_t* Y, int64_t ldy, const uint16_t* W, int64_t ldw, const int64_t* targets, float* nll,
                        float* lse, int64_t M, int64_t V, int64_t K, void* workspace, size_t workspace_bytes, void* stream);

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

/* ---- device-scalar scaling (chunked lm_head + cross-entropy, models/transformer.py:114 + engine/engine.py:111,118)
 * The chunked head runs its dX / dW GEMMs inside forward, before autograd hands over the upstream gradient g
 * (engine.py:118 `(loss / accum).backward()`); backward applies g with
 *   plm_scale_bf16: x[i] <- bf16(x[i] * *alpha_dev)                       (n elements, in place)
 *   plm_axpy_f32:   out[i] <- (accumulate ? out[i] : 0) + *alpha_dev * x[i]  (alpha_dev NULL = 1.0) */
int plm_scale_bf16(uint16_t* x, int64_t n, const float* alpha_dev, void* stream);
int plm_axpy_f32(float* out, const float* x, int64_t n, const float* alpha_dev, int accumulate, void* stream);

/* ---- optimizer tail (engine/engine.py:126-135, optim/init_optim.py:7-70)
 * sumsq: out[0] = sum(x^2) (single-launch deterministic two-stage reduce; scratch >= 4096 floats) */
int plm_sumsq_f32(const float* x, int64_t n, float* scratch, float* out, void* stream);
/* The reference's optimizers, selected by h->kind, on two launch shapes: plm_optim_f32 on a flat fp32 span, and
 * plm_optim_cast_multi on a list of Linear weights [rows, cols] that ALSO writes the bf16 shadows the next step's GEMMs read
 * (dst = bf16(W) [rows, cols], dst_t = bf16(W)^T [cols, ld_t], columns 0..rows-1), i.e. plm_optim_f32 followed by
 * plm_cast_f32_bf16_t_multi in one pass over the parameters ("bf16 weight shadow copy emitted by the
 * optimizer"; replaces the per-call fp32 -> bf16 weight casts of autocast, engine/engine.py:75).  g is pre-multiplied by
 * *clip_coef_dev (NULL = 1); the two forms give the same bits per element.  Scalars are host-computed per group and step:
 *   PLM_OPTIM_ADAMW    torch.optim.AdamW (decoupled decay; bc1 = 1 - b1^t, bc2 = 1 - b2^t):
 *     p *= 1 - lr*wd ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
 *     (the entry points form 1 - lr*wd as fmaf(-lr, wd, 1), lr / bc1 and sqrt(bc2) in fp32 from the struct's lr, weight_decay,
 *     bc1, bc2; decay, coef_grad and coef_avg are ignored; needs m and v)
 *   PLM_OPTIM_NADAMW   torch.optim.NAdam(decoupled_weight_decay=True):
 *     p *= decay ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; d = sqrt(v / bc2) + eps ;
 *     p -= coef_grad * g / d + coef_avg * m / d
 *     (coef_grad = lr (1 - mu_t) / (1 - prod mu), coef_avg = lr mu_{t+1} / (1 - prod mu * mu_{t+1}); needs m and v)
 *   PLM_OPTIM_SGD      torch.optim.SGD(momentum, dampening, weight_decay), nesterov off (coupled L2):
 *     d = g + weight_decay p ; momentum != 0: m = first ? d : momentum m + (1-dampening) d, p -= lr m ;
 *     momentum == 0: p -= lr d (m is neither read nor written and may be NULL); v must be NULL
 *   PLM_OPTIM_SIGNSGD  the reference's optim/signSGD.py:
 *     p *= decay ; m = momentum (first ? g : m) + (1-dampening) g ; p -= lr sign(m)  (sign(0) = 0); v must be NULL
 *   PLM_OPTIM_SFO_ADAMW  schedule-free AdamW (Defazio et al. 2024, the schedulefree package's AdamWScheduleFree), p = y,
 *     m = z, v = exp_avg_sq:
 *     v = b2 v + (1-b2) g^2 ; gn = g / (sqrt(v / bc2) + eps) + weight_decay y ;
 *     y = lerp(y, z, ckp1) + coef_y gn ; z -= lr gn   (the lerp reads the old z; lerp as torch.lerp spells it)
 *     (lr = the warmed-up scheduled_lr, ckp1 = weight / weight_sum, coef_y = lr (b1 (1 - ckp1) - 1); needs m and v)
 * `first` = 1 initialises the momentum buffer (SGD: torch's missing momentum_buffer; signSGD: the missing 'm'; schedule-free
 * AdamW: z = a copy of p and v = 0, neither read).
 * decay (all kinds but AdamW) = 1 - lr * weight_decay, rounded once from the host's double, as torch passes it to p.mul_().
 * rows, cols and ld_t are positive multiples of 8 below 2^31, ld_t >= rows, every pointer is 16-byte aligned.  An unknown kind
 * (0, what a zeroed struct carries, included), a missing or superfluous state buffer, or a bad shape / alignment gives
 * PLM_E_INVALID.  The multi-tensor entry points (this one and plm_cast_f32_bf16_t_multi) validate EVERY item before their first
 * launch, whatever the length of the list: a refused list leaves all parameters as they were. */
#define PLM_OPTIM_NADAMW 1
#define PLM_OPTIM_SGD 2
#define PLM_OPTIM_SIGNSGD 3
#define PLM_OPTIM_SFO_ADAMW 4
#define PLM_OPTIM_ADAMW 5
typedef struct plm_optim_hparams {
  int kind;   /* PLM_OPTIM_* */
  int first;  /* 1: initialise the state buffers this step (SGD / signSGD / schedule-free AdamW) */
  float lr, weight_decay, decay, beta1, beta2, eps, momentum, dampening;
  float bc2, coef_grad, coef_avg; /* NAdamW (bc2 also AdamW and schedule-free AdamW) */
  float ckp1, coef_y;             /* schedule-free AdamW */
  float bc1;                      /* AdamW */
} plm_optim_hparams;
typedef struct plm_optim_item {
  float* p;         /* fp32 [rows, cols], updated in place */
  const float* g;   /* fp32 gradient */
  float* m;         /* exp_avg / momentum buffer / z (NULL for SGD without momentum) */
  float* v;         /* exp_avg_sq (NULL for SGD / signSGD) */
  uint16_t* dst;    /* bf16 [rows, cols] */
  uint16_t* dst_t;  /* bf16 [cols, ld_t] */
  int64_t rows, cols, ld_t;
} plm_optim_item;
int plm_optim_f32(const plm_optim_hparams* h, float* p, const float* g, float* m, float* v, int64_t n,
                  const float* clip_coef_dev, void* stream);
int plm_optim_cast_multi(const plm_optim_hparams* h, const plm_optim_item* items, int count, const float* clip_coef_dev,
                         void* stream);
/* Schedule-free train / eval swap on a flat fp32 span: p[i] = lerp(p[i], z[i], w), as torch.lerp
 * (|w| < 0.5: p + w (z - p), else z - (z - p)(1 - w)).  eval(): w = 1 - 1/beta1 (p = x); train(): w = 1 - beta1 (p = y).
 * A NULL p or z or n <= 0 gives PLM_E_INVALID. */
int plm_lerp_f32(float* p, const float* z, int64_t n, float w, void* stream);

/* ---- Muon for the block matrices: torch.optim.Muon's arithmetic on whole 2-D weights
 * Batched NT GEMM: one launch per PLM_NT_BATCH_GROUP problems, each
 *   C[M,N] = bf16(alpha * (A[M,K] . B[N,K]^T) + beta * float(D[M,N]))     fp32 sums, one rounding per element:
 *   fmaf(alpha, acc, beta * d) with D, alpha * acc without (D NULL; beta is then ignored)
 * and, when Ct is not NULL, Ct[N, ldct] = C^T (the same bits).  Shapes and leading dimensions are per problem: M, N, K and every ld
 * are positive multiples of 8 below 2^31, lda / ldb >= K, ldc / ldd >= N, ldct >= M; every base is 16-byte aligned.  Edge tiles are
 * handled; nothing outside [M, N] of C / [N, M] of Ct is written and nothing outside the stated extents is read.  D may be C itself
 * (each element is read before it is written, by the thread that writes it); A and B must not overlap C or Ct, nor D Ct.  EVERY item is
 * validated before the first launch: a refused list (PLM_E_INVALID) leaves all outputs as they were. */
#define PLM_NT_BATCH_GROUP 32
typedef struct plm_nt_batch_item {
  const uint16_t* A; int64_t lda;   /* bf16 [M, K] */
  const uint16_t* B; int64_t ldb;   /* bf16 [N, K] */
  uint16_t* C; int64_t ldc;         /* bf16 [M, N] */
  const uint16_t* D; int64_t ldd;   /* bf16 [M, N] or NULL */
  uint16_t* Ct; int64_t ldct;       /* bf16 [N, M] or NULL */
  int64_t M, N, K;
  float alpha, beta;
} plm_nt_batch_item;
int plm_gemm_bf16_nt_batched(const plm_nt_batch_item* items, int count, void* stream);

/* The Muon tail of a list of weights W_i fp32 [rows_i, cols_i] (m_i = min, n_i = max of the two; X is always [m, n], the transpose
 * of a tall weight).  The three calls share one caller-owned workspace of plm_muon_workspace_bytes(rows, cols, count) bytes, 16-byte
 * aligned, laid out as: per matrix, in list order, the bf16 blocks X0 [m, n] | X0t [n, m] | X1 [m, n] | X1t [n, m] | A [m, m] |
 * Bm [m, m], all contiguous; then one fp32 partial sum per 64 x 64 tile of every matrix (in list order).
 *   plm_muon_prepare: g' = *clip_coef_dev * g (NULL = 1); buf = lerp(buf, g', 1 - momentum); U = nesterov ? lerp(g', buf, momentum) :
 *     buf (torch.lerp's two-sided form); Ub = bf16(U); nrm[i] = max(bf16(sqrt(sum float(Ub)^2)), bf16(eps)) with the sum in fp32 in
 *     a fixed order (one partial per 64 x 64 tile, then one ordered final sum: no atomics, two runs give the same bits);
 *     X0 = bf16(float(Ub) / nrm[i]) in the wide orientation, X0t = X0^T.  Two launches per 56 matrices.
 *   plm_muon_orthogonalize: `steps` Newton-Schulz steps on every X of the workspace, three plm_gemm_bf16_nt_batched launches per step
 *     and PLM_NT_BATCH_GROUP matrices:  A = bf16(X X^T) ; Bm = bf16(b A + c (A A)) ; X' = bf16(a X + Bm X), X't = X'^T.
 *     Step s reads X{s & 1} and writes X{(s + 1) & 1}: the result is X{steps & 1} and its transpose.
 *   plm_muon_apply: W = fmaf(-lr_adj_i, float(O), W * decay) with O = the result of `steps` steps read in W's layout (X for a wide
 *     weight, Xt for a tall one; steps = 0 reads X0); dst = bf16(W) and dst_t = bf16(W)^T [cols, ld_t] are written in the same pass.
 * rows, cols, ld_t: positive multiples of 8 below 2^31 (rows * cols < 2^30), ld_t >= rows; all pointers 16-byte aligned; momentum in
 * [0, 1); steps in 1..99 (plm_muon_apply: 0..99); at most 4096 matrices.  PLM_E_INVALID for a refused argument, PLM_E_WORKSPACE for a short or misaligned workspace, both before
 * anything is launched.  plm_muon_workspace_bytes returns 0 for a list it refuses. */
typedef struct plm_muon_item {
  float* p;         /* fp32 [rows, cols], updated in place by plm_muon_apply */
  const float* g;   /* fp32 gradient (plm_muon_prepare) */
  float* buf;       /* fp32 momentum buffer, updated in place by plm_muon_prepare */
  uint16_t* dst;    /* bf16 [rows, cols] (plm_muon_apply) */
  uint16_t* dst_t;  /* bf16 [cols, ld_t] (plm_muon_apply) */
  int64_t rows, cols, ld_t;
  float lr_adj;     /* the shape-adjusted learning rate (plm_muon_apply) */
} plm_muon_item;
size_t plm_muon_workspace_bytes(const int64_t* rows, const int64_t* cols, int count);
int plm_muon_prepare(const plm_muon_item* items, int count, float momentum, int nesterov, float eps, const float* clip_coef_dev,
                     float* nrm, void* workspace, size_t workspace_bytes, void* stream);
int plm_muon_orthogonalize(const int64_t* rows, const int64_t* cols, int count, int steps, float a, float b, float c, void* workspace,
                           size_t workspace_bytes, void* stream);
int plm_muon_apply(const plm_muon_item* items, int count, float decay, int steps, const void* workspace, size_t workspace_bytes,
                   void* stream);

/* ---- MXFP8 (OCP MX: e4m3fn elements, one E8M0 scale byte per 32 elements)
 * Layout of a quantized operand blocked along its K: data uint8 [rows, Kp] and scales uint8 [rows, Kp/32], both row-major, Kp = roundup(K, 128);
 * padding elements are zero with scale byte 0.  Scale rule: amax = max |x| of the block, E = floor(log2 amax), e = E - 8 if amax <= 448 * 2^(E-8)
 * else E - 7, clamped to [-127, 127]; scale byte e + 127, element RNE_e4m3fn(x * 2^-e) (subnormals kept).  amax = 0: scale byte 0, zero
 * elements; a block holding NaN / Inf: scale byte 0xFF, every element 0x7F (NaN), so it reaches the GEMM output as NaN.
 * plm_mx_quant: bf16 x [rows, cols] (leading dimension ld) -> the row-blocked copy q [rows, roundup(cols,128)] + s, and/or the transposed
 * copy qt [cols, roundup(rows,128)] + st blocked along rows, from one read of x.  Either pair may be NULL, not both.  Needs cols % 8 == 0,
 * ld % 8 == 0, x / q / qt 16-byte aligned.  plm_mx_quant_multi: the same for `count` items in one launch (per 64 items). */
typedef struct plm_mx_quant_item {
  const uint16_t* x; /* bf16 [rows, ld] */
  int64_t ld;
  int64_t rows;
  int64_t cols;
  uint8_t* q;  /* [rows, roundup(cols,128)] or NULL */
  uint8_t* s;  /* [rows, roundup(cols,128)/32] or NULL */
  uint8_t* qt; /* [cols, roundup(rows,128)] or NULL */
  uint8_t* st; /* [cols, roundup(rows,128)/32] or NULL */
} plm_mx_quant_item;
int plm_mx_quant(const uint16_t* x, int64_t ld, int64_t rows, int64_t cols, uint8_t* q, uint8_t* s, uint8_t* qt, uint8_t* st, void* stream);
int plm_mx_quant_multi(const plm_mx_quant_item* items, int count, void* stream);
/* C[M,N] = deq(A)[M,Kp] . deq(B)[N,Kp]^T (A, B quantized along Kp as above) on v_mfma_scale_f32_32x32x64_f8f6f4, fp32 accumulation.
 * mode PLM_MX_OUT_BF16: C bf16, PLM_MX_OUT_F32: C fp32 stored, PLM_MX_OUT_F32_ACC: C fp32 += the product (main_grad).  Row stride ldc >= N.
 * Needs Kp % 128 == 0, A / B 16-byte aligned, scales 4-byte aligned. */
#define PLM_MX_OUT_BF16 0
#define PLM_MX_OUT_F32 1
#define PLM_MX_OUT_F32_ACC 2
int plm_gemm_mx_nt(const uint8_t* A, const uint8_t* As, const uint8_t* B, const uint8_t* Bs, void* C, int64_t ldc, int64_t M, int64_t N, int64_t Kp,
                   int mode, void* stream);

/* Leave `n` CUs free when sizing the persistent GEMM grids (one workgroup per CU, static tile schedule), so that
 * concurrently running RCCL collectives do not push GEMM workgroups into a second round.  Process-wide; 0 = whole chip. */
int plm_set_cu_reserve(int n);

/* ---- RCCL data-parallel gradient exchange (replaces DDP: engine/engine.py:64-65,104-105)
 * One communicator per process (one process per GPU).  uid is the 128-byte ncclUniqueId
 * produced by plm_comm_unique_id on rank 0 and shipped to the other ranks by the host. */
typedef struct plm_comm plm_comm_t;
int plm_comm_unique_id(uint8_t uid[128]);
int plm_comm_init(plm_comm_t** comm, const uint8_t uid[128], int rank, int world_size, int device);
/* Same, with a per-communicator cap on the workgroups (= CUs) RCCL may use for one collective (ncclConfig_t.maxCTAs;
 * max_ctas <= 0: RCCL's default).  Gradient buckets reduced WHILE backward is still running go through a capped
 * communicator (the persistent GEMMs leave exactly that many CUs free, plm_set_cu_reserve), the buckets that become ready
 * when backward has ended - embed_tokens, 154 MB, ready last: engine/engine.py:104-105 leaves it exposed too - go through
 * an uncapped one: with nothing left to overlap with, the tail should use every xGMI link.  The host side (plainlm_amd/ddp.py,
 * round 5) creates the UNCAPPED communicator first (plm_comm_init) and splits the capped ones off it (plm_comm_split). */
int plm_comm_init_capped(plm_comm_t** comm, const uint8_t uid[128], int rank, int world_size, int device, int max_ctas);
/* ncclCommSplit of `parent` into a communicator over the same ranks with its own CTA cap (collective over parent's ranks). */
int plm_comm_split(plm_comm_t* parent, plm_comm_t** child, int max_ctas);
int plm_comm_destroy(plm_comm_t* comm);
/* in-place all-reduce-mean of a fp32 span on `stream` (the side stream owned by the caller) */
int plm_comm_allreduce_avg_f32(plm_comm_t* comm, float* buf, int64_t count, void* stream);
/* the same mean as reduce-scatter + all-gather in place (one-hop collectives over all xGMI links; the reducer's `algo` choice -
 * PLM_COMM_ALGO=rsag, or bench.py's autotune) */
int plm_comm_rsag_avg_f32(plm_comm_t* comm, float* buf, int64_t count, void* stream);
int plm_comm_broadcast_f32(plm_comm_t* comm, float* buf, int64_t count, int root, void* stream);

/* ---- hardware probes used by the GPU tests (semantics of gfx950 instructions the kernels rely on)
 * out int32[64*4]: element [lane*4+j] = value lane received in slot j from ds_read_b64_tr_b16 when
 * lane l supplied address base + 8*l bytes and LDS held the uint16 sequence 0,1,2,... */
int plm_probe_ds_read_tr16(int32_t* out, void* stream);
/* out fp32[32*32] = A·B for A[32,16], B[16,32] given as fp32 row-major (rounded to bf16), one wave */
int plm_probe_mfma32(const float* A, const float* B, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PLAINLM_HIP_H */
