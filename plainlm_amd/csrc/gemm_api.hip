// The C entry points of the bf16 GEMMs (include/plainlm_hip.h).  Each one validates its arguments, makes ONE plan (gemm_plan.h) from the shape,
// the persistent grid size and the environment switches, and hands that plan to the workspace check and to a launch function of a kernel
// file (gemm_launch.h): no kernel lives here, and no kernel file decides anything.
#include <initializer_list>

#include "../../include/plainlm_hip.h"
#include "gemm_launch.h"

static int g_num_cus = 0;
static int g_cu_reserve = 0;  // CUs left free for concurrent kernels (RCCL collectives during backward)

// The persistent GEMMs launch one workgroup per CU with a static tile schedule.  A concurrent kernel that occupies
// some CUs (RCCL's all-reduce on the side stream) would push the displaced workgroups into a second round; leaving
// `n` CUs free avoids that.  Process-wide setting; 0 restores the full chip.
extern "C" int plm_set_cu_reserve(int n) {
  if (n < 0 || n > 128) {
    plm_set_error("plm_set_cu_reserve: n=%d out of range 0..128", n);
    return PLM_E_INVALID;
  }
  g_cu_reserve = n;
  return PLM_OK;
}

static bool ensure_num_cus() {
  if (g_num_cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    g_num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  return true;
}

// number of persistent workgroups to launch: one per CU minus the reserve.  0 (and the error string set): no device to ask
static int persistent_slots() {
  if (!ensure_num_cus()) {
    plm_set_error("bf16 GEMM: cannot query the HIP device for its CU count");
    return 0;
  }
  const int n = g_num_cus - g_cu_reserve;
  return n < 8 ? 8 : n;
}

static GemmPlanEnv plan_env() {
  const PlmEnv& e = plm_env();
  return GemmPlanEnv{e.gemm_v1, e.tn_no_big, e.nt_no_hybrid, e.nt_hybrid_min_k};
}

// 16-byte alignment of every pointer a fused launch touches with 16-byte vector accesses (LDS-DMA sources, row stores, the saved fc1 output,
// the RoPE tables): a caller of the C ABI with a misaligned view gets the two-launch fallback (whose GEMM checks its own operands), not a
// misaligned global_load_lds_dwordx4
static bool aligned16(std::initializer_list<const void*> ptrs) {
  uintptr_t v = 0;
  for (const void* p : ptrs) v |= reinterpret_cast<uintptr_t>(p);
  return (v & 15) == 0;
}

// ---------------------------------------------------------------------------------------------
// NT
// ---------------------------------------------------------------------------------------------
// The launch uses these slabs only when it is handed a workspace of at least this size AND plans the hybrid itself; the query answers for
// the hybrid schedule alone, so it can be > 0 for a launch that will not use it (PLM_GEMM_V1, an fp32 C, an ldc that is no multiple of 8).
// The asymmetry is as old as the query and harmless (an unused buffer); hence PLM_GEMM_V1 is not passed on here.
extern "C" size_t plm_gemm_nt_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  const int slots = persistent_slots();
  if (M <= 0 || N <= 0 || K <= 0 || slots == 0) return 0;
  GemmPlanEnv env = plan_env();
  env.gemm_v1 = false;
  return nt_plan(M, N, K, N, 0, 0, true, NT_EPI_NONE, slots, env).workspace_bytes;
}

extern "C" int plm_gemm_bf16_nt_ws(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, void* C, int64_t ldc, int64_t M,
                                   int64_t N, int64_t K, int c_dtype, int accumulate, const float* alpha_dev, int variant,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  PLM_REQUIRE(A && B && C, "plm_gemm_bf16_nt: null pointer");
  PLM_REQUIRE(variant >= 0 && variant <= 7, "plm_gemm_bf16_nt_ex: variant must be 0..7");
  PLM_REQUIRE(M > 0 && N > 0 && K > 0 && M < (1 << 30) && N < (1 << 30) && K < (1 << 30), "plm_gemm_bf16_nt: bad shape M=%ld N=%ld K=%ld",
              (long)M, (long)N, (long)K);
  PLM_REQUIRE(K % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc % 4 == 0, "plm_gemm_bf16_nt: K, lda, ldb must be multiples of 8 and ldc of 4 (K=%ld lda=%ld ldb=%ld ldc=%ld)",
              (long)K, (long)lda, (long)ldb, (long)ldc);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(C)) & 15) == 0,
              "plm_gemm_bf16_nt: base pointers must be 16-byte aligned");
  PLM_REQUIRE(c_dtype == 0 || c_dtype == 1, "plm_gemm_bf16_nt: c_dtype must be 0 (bf16) or 1 (fp32)");
  PLM_REQUIRE(!(accumulate && c_dtype == 0), "plm_gemm_bf16_nt: accumulate needs an fp32 C");
  PLM_REQUIRE(variant <= 1 || nt_dma_shape(N, K, ldc), "plm_gemm_bf16_nt_ex: variant %d needs K %% 64 == 0, N %% 8 == 0, ldc %% 8 == 0", variant);
  PLM_REQUIRE(variant <= 2 || c_dtype == 0, "plm_gemm_bf16_nt_ex: the big-tile variants write bf16 C only");
  const int slots = persistent_slots();
  if (slots == 0) return PLM_E_HIP;
  NtPlan p = nt_plan(M, N, K, ldc, c_dtype, variant, workspace != nullptr, NT_EPI_NONE, slots, plan_env());
  if (p.workspace_bytes > workspace_bytes)  // a workspace too small for the hybrid's slabs: the plain schedules
    p = nt_plan(M, N, K, ldc, c_dtype, variant, false, NT_EPI_NONE, slots, plan_env());
  const GemmOperands o{A, lda, B, ldb, C, ldc, M, N, K, alpha_dev};
  if (p.kernel == NT_PERSISTENT || p.kernel == NT_HYBRID) {
    plm_launch_gemm_nt_persistent(p, NT_EPI_NONE, o, (float*)workspace, EpiArgs{}, (hipStream_t)stream);
    PLM_CHECK_LAUNCH("plm_gemm_bf16_nt (big tile)");
    return PLM_OK;
  }
  plm_launch_gemm_nt_128(p, o, c_dtype, accumulate, (hipStream_t)stream);
  PLM_CHECK_LAUNCH("plm_gemm_bf16_nt");
  return PLM_OK;
}

extern "C" int plm_gemm_bf16_nt_ex(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, void* C, int64_t ldc, int64_t M,
                                   int64_t N, int64_t K, int c_dtype, int accumulate, const float* alpha_dev, int variant,
                                   void* stream) {
  return plm_gemm_bf16_nt_ws(A, lda, B, ldb, C, ldc, M, N, K, c_dtype, accumulate, alpha_dev, variant, nullptr, 0, stream);
}

extern "C" int plm_gemm_bf16_nt(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, void* C, int64_t ldc, int64_t M,
                                int64_t N, int64_t K, int c_dtype, int accumulate, const float* alpha_dev, void* stream) {
  return plm_gemm_bf16_nt_ws(A, lda, B, ldb, C, ldc, M, N, K, c_dtype, accumulate, alpha_dev, 0, nullptr, 0, stream);
}

// The fused epilogues: one launch on the persistent kernel when nt_plan qualifies the shape.  false: the caller takes its two-launch path
// (same bits).  The callers check the leading dimensions and the alignment of every pointer the fused kernel touches with 16-byte accesses.
static bool launch_nt_fused(NtEpilogue epilogue, const GemmOperands& o, const EpiArgs& ea, void* stream) {
  const int slots = persistent_slots();
  if (slots == 0) return false;
  const NtPlan p = nt_plan(o.M, o.N, o.K, o.ldc, 0, 0, false, epilogue, slots, plan_env());
  if (p.ok) plm_launch_gemm_nt_persistent(p, epilogue, o, nullptr, ea, (hipStream_t)stream);
  return p.ok;
}

// w_qkv projection with RoPE: qkv[M, 3*nh*hd] = x W^T with the q | k column blocks rotated (row m = position m % T) in the GEMM
// epilogue: the 16-byte chunks are rotated on their way from the transposition scratch to memory, one 16-byte table read per
// table and chunk (round 1 rotated accumulator fragments - per-lane table gathers, 58 us per call - and lost to the 31 us
// stand-alone pass, which remains the fallback: same bits).
extern "C" int plm_qkv_rope_bf16(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, uint16_t* QKV, int64_t ldq, int64_t M,
                                 int64_t K, const float* rope_cos, const float* rope_sin, int64_t B, int64_t T, int64_t nh, int64_t hd,
                                 void* stream) {
  PLM_REQUIRE(X && W && QKV && rope_cos && rope_sin, "plm_qkv_rope_bf16: null pointer");
  PLM_REQUIRE((hd == 64 || hd == 32 || hd == 128) && B > 0 && T > 0 && nh > 0 && M == B * T, "plm_qkv_rope_bf16: bad shape (hd 32 / 64 / 128, M == B*T)");
  const int64_t N = 3 * nh * hd;
  PLM_REQUIRE(ldq == N, "plm_qkv_rope_bf16: needs a dense output (ldq == 3*nh*hd)");
  // the store-side rotation is built for 64-wide heads; other head dims take GEMM + the stand-alone pass
  if (hd == 64 && ldx % 8 == 0 && ldw % 8 == 0 && aligned16({X, W, QKV, rope_cos, rope_sin}) &&
      launch_nt_fused(NT_EPI_ROPE, GemmOperands{X, ldx, W, ldw, QKV, ldq, M, N, K, nullptr},
                      EpiArgs{nullptr, 0, rope_cos, rope_sin, (int)T, (int)(2 * nh * hd)}, stream)) {
    PLM_CHECK_LAUNCH("plm_qkv_rope_bf16");
    return PLM_OK;
  }
  if (int rc = plm_gemm_bf16_nt_ex(X, ldx, W, ldw, QKV, ldq, M, N, K, 0, 0, nullptr, 0, stream)) return rc;
  return plm_rope_qk(QKV, rope_cos, rope_sin, B, T, nh, hd, stream);
}

// fc1 of the SwiGLU MLP with the activation in the GEMM epilogue (models/components.py:50-56):
//   U[M, 2h] = X[M, K] W[2h, K]^T  (gate | up, kept for backward)  and  ACT[M, h] = bf16(bf16(silu(gate)) * up).
// One launch on the persistent 256x256 kernel when the shape qualifies (2h % 256 == 0, K % 64 == 0, M >= 512); otherwise the GEMM
// followed by plm_swiglu_fwd - the two paths produce the same bits.
extern "C" int plm_fc1_swiglu_bf16(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, uint16_t* U, uint16_t* ACT, int64_t M,
                                   int64_t h, int64_t K, void* stream) {
  PLM_REQUIRE(X && W && U && ACT, "plm_fc1_swiglu_bf16: null pointer");
  PLM_REQUIRE(M > 0 && h > 0 && K > 0 && h % 8 == 0, "plm_fc1_swiglu_bf16: bad shape (h %% 8 == 0)");
  const int64_t N = 2 * h;
  if (ldx % 8 == 0 && ldw % 8 == 0 && aligned16({X, W, U, ACT}) &&  // (the rows of U and ACT: N and h are multiples of 8)
      launch_nt_fused(NT_EPI_GLU, GemmOperands{X, ldx, W, ldw, U, N, M, N, K, nullptr}, EpiArgs{ACT, h, nullptr, nullptr, 0, 0}, stream)) {
    PLM_CHECK_LAUNCH("plm_fc1_swiglu_bf16");
    return PLM_OK;
  }
  if (int rc = plm_gemm_bf16_nt_ex(X, ldx, W, ldw, U, N, M, N, K, 0, 0, nullptr, 0, stream)) return rc;
  return plm_swiglu_fwd(U, ACT, M, h, stream);
}

// Backward of the SwiGLU MLP's second half (models/components.py:55-57): d(act)[M, h] = dY[M, K] W2T[h, K]^T never reaches memory -
// the epilogue of that GEMM applies the SwiGLU backward with the saved fc1 output U[M, 2h] and writes DU[M, 2h] (d(gate) | d(up)).
// One launch when h % 256 == 0, K % 64 == 0, M >= 512; otherwise the GEMM followed by plm_swiglu_bwd (same bits; `scratch` must then
// hold M*h bf16 values for d(act), it is not touched by the fused path and may be NULL when the shape qualifies).
extern "C" int plm_fc2_dx_swiglu_bwd_bf16(const uint16_t* dY, int64_t lddy, const uint16_t* W2T, int64_t ldw, const uint16_t* U, uint16_t* DU,
                                          uint16_t* scratch, int64_t M, int64_t h, int64_t K, void* stream) {
  PLM_REQUIRE(dY && W2T && U && DU, "plm_fc2_dx_swiglu_bwd_bf16: null pointer");
  PLM_REQUIRE(M > 0 && h > 0 && K > 0 && h % 8 == 0, "plm_fc2_dx_swiglu_bwd_bf16: bad shape (h %% 8 == 0)");
  // U is read in 8-byte pieces (its rows and DU's are 2h long: a multiple of 8)
  if (lddy % 8 == 0 && ldw % 8 == 0 && aligned16({dY, W2T, DU}) && (reinterpret_cast<uintptr_t>(U) & 7) == 0 &&
      launch_nt_fused(NT_EPI_GLUB, GemmOperands{dY, lddy, W2T, ldw, DU, 2 * h, M, h, K, nullptr},
                      EpiArgs{const_cast<uint16_t*>(U), 2 * h, nullptr, nullptr, 0, 0}, stream)) {
    PLM_CHECK_LAUNCH("plm_fc2_dx_swiglu_bwd_bf16");
    return PLM_OK;
  }
  if (!scratch) {  // not an error of the shape: the caller retries with the buffer
    plm_set_error("plm_fc2_dx_swiglu_bwd_bf16: this shape (or PLM_GEMM_V1) takes the two-launch path and needs the M*h bf16 d(act) scratch");
    return PLM_E_WORKSPACE;
  }
  if (int rc = plm_gemm_bf16_nt_ex(dY, lddy, W2T, ldw, scratch, h, M, h, K, 0, 0, nullptr, 0, stream)) return rc;
  return plm_swiglu_bwd(scratch, U, DU, M, h, stream);
}

// ---------------------------------------------------------------------------------------------
// TN
// ---------------------------------------------------------------------------------------------
extern "C" size_t plm_gemm_tn_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  const int slots = persistent_slots();
  if (M <= 0 || N <= 0 || K <= 0 || slots == 0) return 0;
  return tn_plan(M, N, K, slots, plan_env()).workspace_bytes;
}

extern "C" int plm_gemm_bf16_tn(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, float* C, int64_t ldc, int64_t M,
                                int64_t N, int64_t K, int accumulate, const float* alpha_dev, void* workspace,
                                size_t workspace_bytes, void* stream) {
  PLM_REQUIRE(A && B && C, "plm_gemm_bf16_tn: null pointer");
  PLM_REQUIRE(M > 0 && N > 0 && K > 0 && M < (1 << 30) && N < (1 << 30) && K < (1 << 30), "plm_gemm_bf16_tn: bad shape M=%ld N=%ld K=%ld",
              (long)M, (long)N, (long)K);
  PLM_REQUIRE(M % 8 == 0 && N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ldc % 4 == 0,
              "plm_gemm_bf16_tn: M, N, lda, ldb must be multiples of 8 and ldc of 4 (M=%ld N=%ld lda=%ld ldb=%ld ldc=%ld)", (long)M, (long)N,
              (long)lda, (long)ldb, (long)ldc);
  PLM_REQUIRE(((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(C)) & 15) == 0,
              "plm_gemm_bf16_tn: base pointers must be 16-byte aligned");
  const int slots = persistent_slots();
  if (slots == 0) return PLM_E_HIP;
  const TnPlan p = tn_plan(M, N, K, slots, plan_env());
  if (p.splits > 1) {
    if (!workspace || workspace_bytes < p.workspace_bytes) {
      plm_set_error("plm_gemm_bf16_tn: workspace of %zu bytes required, %zu given", p.workspace_bytes, workspace_bytes);
      return PLM_E_WORKSPACE;
    }
    PLM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "plm_gemm_bf16_tn: workspace must be 16-byte aligned");
  }
  const GemmOperands o{A, lda, B, ldb, C, ldc, M, N, K, alpha_dev};
  (p.kernel == TN_PERSISTENT ? plm_launch_gemm_tn_persistent : plm_launch_gemm_tn_128)(p, o, accumulate, (float*)workspace, (hipStream_t)stream);
  if (p.splits > 1) plm_launch_splitk_reduce(p, o, accumulate, (float*)workspace, (hipStream_t)stream);
  PLM_CHECK_LAUNCH(p.kernel == TN_PERSISTENT ? "plm_gemm_bf16_tn (big tile)" : "plm_gemm_bf16_tn");
  return PLM_OK;
}

// ---- grouped TN (dW of one or more transformer blocks in one launch, see GROUPED in gemm_big.hip) ----
extern "C" size_t plm_gemm_tn_grouped_workspace_bytes(const int64_t* Ms, const int64_t* Ns, int count, int64_t K) {
  TnGroup g{};
  size_t need = 0;
  const int slots = persistent_slots();
  if (!Ms || !Ns || slots == 0 || !tn_group_plan(Ms, Ns, count, K, slots, &g, &need)) return 0;
  return need + 16;  // never zero: 0 means "unsupported shapes"
}

extern "C" int plm_gemm_bf16_tn_grouped(const plm_tn_problem* probs, int count, int64_t K, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  PLM_REQUIRE(probs && workspace, "plm_gemm_bf16_tn_grouped: null pointer");
  PLM_REQUIRE(count >= 1 && count <= PLM_TN_GROUP_MAX, "plm_gemm_bf16_tn_grouped: count=%d must be 1..%d", count, PLM_TN_GROUP_MAX);
  int64_t Ms[PLM_TN_GROUP_MAX], Ns[PLM_TN_GROUP_MAX];
  TnGroup g{};
  TnGroupOut o{};
  for (int p = 0; p < count; ++p) {
    const plm_tn_problem& q = probs[p];
    PLM_REQUIRE(q.A && q.B && q.C, "plm_gemm_bf16_tn_grouped: null pointer in problem %d", p);
    PLM_REQUIRE(q.M % 8 == 0 && q.N % 8 == 0 && q.lda % 8 == 0 && q.ldb % 8 == 0 && q.ldc % 4 == 0 && q.lda >= q.M && q.ldb >= q.N && q.ldc >= q.N,
                "plm_gemm_bf16_tn_grouped: problem %d: M, N, lda, ldb must be multiples of 8, ldc of 4", p);
    PLM_REQUIRE(q.lda < (1ll << 31) && q.ldb < (1ll << 31) && q.ldc < (1ll << 31), "plm_gemm_bf16_tn_grouped: problem %d: row strides must fit 31 bits", p);
    PLM_REQUIRE(((reinterpret_cast<uintptr_t>(q.A) | reinterpret_cast<uintptr_t>(q.B) | reinterpret_cast<uintptr_t>(q.C)) & 15) == 0,
                "plm_gemm_bf16_tn_grouped: problem %d: base pointers must be 16-byte aligned", p);
    Ms[p] = q.M;
    Ns[p] = q.N;
    g.A[p] = q.A;
    g.B[p] = q.B;
    g.lda[p] = (int)q.lda;
    g.ldb[p] = (int)q.ldb;
    o.C[p] = q.C;
    o.ldc[p] = (int)q.ldc;
    o.alpha[p] = q.alpha_dev;
    o.accumulate[p] = q.accumulate;
  }
  const int slots = persistent_slots();
  if (slots == 0) return PLM_E_HIP;
  size_t need = 0;
  PLM_REQUIRE(tn_group_plan(Ms, Ns, count, K, slots, &g, &need), "plm_gemm_bf16_tn_grouped: unsupported shapes (K %% 64 == 0, M, N multiples of 8)");
  if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0) {
    plm_set_error("plm_gemm_bf16_tn_grouped: workspace of %zu bytes (16-byte aligned) required, %zu given", need, workspace_bytes);
    return PLM_E_WORKSPACE;
  }
  plm_launch_gemm_tn_grouped(g, o, K, (float*)workspace, slots, (hipStream_t)stream);
  PLM_CHECK_LAUNCH("plm_gemm_bf16_tn_grouped");
  return PLM_OK;
}

// =============================================================================================
// Forward-only scoring head:  nll[M], lse[M] of  softmax(bf16(Y W^T))  without the [M, V] logits
// =============================================================================================
// Workspace: xt fp32[M] | then EITHER the row partials [ceil(V / BN)][M] (max, sum-exp) of the persistent kernel OR the logits of
// PLM_HS_CHUNK rows (shapes the automatic policy of plm_gemm_bf16_nt gives to a 128x128 kernel: M < 512, V % 8 != 0, badly quantised
// grids).  The query does not know the device, so it sizes the partials for the narrowest tile (BN = 128).
#define PLM_HS_CHUNK 256
static size_t hs_align(size_t n) { return (n + 255) & ~(size_t)255; }
static size_t hs_xt_bytes(int64_t M) { return hs_align((size_t)M * sizeof(float)); }

extern "C" size_t plm_head_score_workspace_bytes(int64_t M, int64_t V, int64_t K) {
  if (M <= 0 || V <= 0 || K <= 0) return 0;
  const size_t part = (size_t)M * (size_t)plm_cdiv(V, 128) * 2 * sizeof(float);
  const size_t chunk = (size_t)PLM_HS_CHUNK * (size_t)(plm_cdiv(V, 8) * 8) * sizeof(uint16_t);
  return hs_xt_bytes(M) + hs_align(part > chunk ? part : chunk);
}

extern "C" int plm_head_score_bf16(const uint16_t* Y, int64_t ldy, const uint16_t* W, int64_t ldw, const int64_t* targets, float* nll,
                                   float* lse, int64_t M, int64_t V, int64_t K, void* workspace, size_t workspace_bytes, void* stream) {
  PLM_REQUIRE(Y && W && targets && nll && workspace, "plm_head_score_bf16: null pointer");
  PLM_REQUIRE(M > 0 && V > 0 && K > 0 && M < (1 << 30) && V < (1 << 30) && K < (1 << 30), "plm_head_score_bf16: bad shape M=%ld V=%ld K=%ld",
              (long)M, (long)V, (long)K);
  PLM_REQUIRE(K % 64 == 0, "plm_head_score_bf16: K %% 64 == 0 required (K=%ld)", (long)K);
  PLM_REQUIRE(ldy % 8 == 0 && ldw % 8 == 0 && ldy >= K && ldw >= K, "plm_head_score_bf16: row strides must be multiples of 8 and >= K (ldy=%ld ldw=%ld)",
              (long)ldy, (long)ldw);
  PLM_REQUIRE(aligned16({Y, W, workspace}) && ((reinterpret_cast<uintptr_t>(nll) | reinterpret_cast<uintptr_t>(lse)) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(targets) & 7) == 0,
              "plm_head_score_bf16: Y, W and the workspace must be 16-byte aligned, targets 8-byte, nll / lse 4-byte");
  const size_t need = plm_head_score_workspace_bytes(M, V, K);
  if (workspace_bytes < need) {
    plm_set_error("plm_head_score_bf16: workspace of %zu bytes required, %zu given", need, workspace_bytes);
    return PLM_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* xt = (float*)workspace;
  char* rest = (char*)workspace + hs_xt_bytes(M);
  // the tile shape plm_gemm_bf16_nt picks for this shape (no workspace: its stream-K hybrid is for K >= 8192), so that the accumulators
  // are the ones the training head rounds to bf16: the same nt_plan, asked for the SCORE epilogue
  const int64_t ld = plm_cdiv(V, 8) * 8;
  const int slots = persistent_slots();
  if (slots == 0) return PLM_E_HIP;
  const NtPlan p = nt_plan(M, V, K, ld, 0, 0, false, NT_EPI_SCORE, slots, plan_env());
  if (p.ok) {
    plm_launch_gemm_nt_persistent(p, NT_EPI_SCORE, GemmOperands{Y, ldy, W, ldw, nullptr, 0, M, V, K, nullptr}, nullptr,
                                  EpiArgs{nullptr, 0, nullptr, nullptr, 0, 0, targets, (float*)rest, xt}, s);
    plm_launch_head_score_combine((const float*)rest, xt, targets, nll, lse, M, V, p.tn, s);
    PLM_CHECK_LAUNCH("plm_head_score_bf16");
    return PLM_OK;
  }
  // shapes plm_gemm_bf16_nt serves with a 128x128 kernel: that kernel (named explicitly, so that a chunk of rows gets the accumulators the
  // whole matrix would) into PLM_HS_CHUNK rows of logits, then the row kernel
  const int variant = p.kernel == NT_DMA128 ? 2 : 1;
  for (int64_t r0 = 0; r0 < M; r0 += PLM_HS_CHUNK) {
    const int64_t rows = M - r0 < PLM_HS_CHUNK ? M - r0 : PLM_HS_CHUNK;
    const int rc = plm_gemm_bf16_nt_ws(Y + r0 * ldy, ldy, W, ldw, rest, ld, rows, V, K, 0, 0, nullptr, variant, nullptr, 0, stream);
    if (rc != PLM_OK) return rc;
    plm_launch_head_score_rows((const uint16_t*)rest, ld, targets + r0, nll + r0, lse ? lse + r0 : nullptr, rows, V, s);
  }
  PLM_CHECK_LAUNCH("plm_head_score_bf16");
  return PLM_OK;
}

// =============================================================================================
// Prediction head (include/plainlm_hip.h):  pred[M], logp[M], entropy[M] (and nll / lse as above) without the logits
// =============================================================================================
// Workspace: xt fp32[M] | then EITHER the 16-byte row records [ceil(V / BN)][M] of the persistent kernel's prediction mode OR the logits of
// PLM_HS_CHUNK rows - plm_head_score_bf16's layout with records twice as large, sized for the narrowest tile (BN = 128) as well.
extern "C" size_t plm_head_predict_workspace_bytes(int64_t M, int64_t V, int64_t K) {
  if (M <= 0 || V <= 0 || K <= 0) return 0;
  const size_t part = (size_t)M * (size_t)plm_cdiv(V, 128) * 4 * sizeof(float);
  const size_t chunk = (size_t)PLM_HS_CHUNK * (size_t)(plm_cdiv(V, 8) * 8) * sizeof(uint16_t);
  return hs_xt_bytes(M) + hs_align(part > chunk ? part : chunk);
}

extern "C" int plm_head_predict_bf16(const uint16_t* Y, int64_t ldy, const uint16_t* W, int64_t ldw, const int64_t* targets, int64_t* pred,
                                     float* logp, float* entropy, float* nll, float* lse, int64_t M, int64_t V, int64_t K, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  PLM_REQUIRE(Y && W && pred && logp && workspace, "plm_head_predict_bf16: null pointer");
  PLM_REQUIRE(targets || !nll, "plm_head_predict_bf16: null pointer (nll needs targets)");
  PLM_REQUIRE(M > 0 && V > 0 && K > 0 && M < (1 << 30) && V < (1 << 30) && K < (1 << 30), "plm_head_predict_bf16: bad shape M=%ld V=%ld K=%ld",
              (long)M, (long)V, (long)K);
  PLM_REQUIRE(K % 64 == 0, "plm_head_predict_bf16: K %% 64 == 0 required (K=%ld)", (long)K);
  PLM_REQUIRE(ldy % 8 == 0 && ldw % 8 == 0 && ldy >= K && ldw >= K, "plm_head_predict_bf16: row strides must be multiples of 8 and >= K (ldy=%ld ldw=%ld)",
              (long)ldy, (long)ldw);
  PLM_REQUIRE(aligned16({Y, W, workspace}) &&
                  ((reinterpret_cast<uintptr_t>(logp) | reinterpret_cast<uintptr_t>(entropy) | reinterpret_cast<uintptr_t>(nll) |
                    reinterpret_cast<uintptr_t>(lse)) & 3) == 0 &&
                  ((reinterpret_cast<uintptr_t>(targets) | reinterpret_cast<uintptr_t>(pred)) & 7) == 0,
              "plm_head_predict_bf16: Y, W and the workspace must be 16-byte aligned, targets / pred 8-byte, logp / entropy / nll / lse 4-byte");
  const size_t need = plm_head_predict_workspace_bytes(M, V, K);
  if (workspace_bytes < need) {
    plm_set_error("plm_head_predict_bf16: workspace of %zu bytes required, %zu given", need, workspace_bytes);
    return PLM_E_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* xt = (float*)workspace;
  char* rest = (char*)workspace + hs_xt_bytes(M);
  // the plan of plm_head_score_bf16 (= the one plm_gemm_bf16_nt makes for this shape): the same accumulators, hence the same bf16 logits
  const int64_t ld = plm_cdiv(V, 8) * 8;
  const int slots = persistent_slots();
  if (slots == 0) return PLM_E_HIP;
  const NtPlan p = nt_plan(M, V, K, ld, 0, 0, false, NT_EPI_SCORE, slots, plan_env());
  const HeadPredictOut out{pred, logp, entropy, nll, lse};
  if (p.ok) {
    plm_launch_gemm_nt_persistent(p, NT_EPI_SCORE, GemmOperands{Y, ldy, W, ldw, nullptr, 0, M, V, K, nullptr}, nullptr,
                                  EpiArgs{nullptr, 0, nullptr, nullptr, 0, 0, targets, nullptr, xt, (float*)rest}, s);
    plm_launch_head_predict_combine((const float*)rest, xt, targets, out, M, V, p.tn, s);
    PLM_CHECK_LAUNCH("plm_head_predict_bf16");
    return PLM_OK;
  }
  const int variant = p.kernel == NT_DMA128 ? 2 : 1;
  for (int64_t r0 = 0; r0 < M; r0 += PLM_HS_CHUNK) {
    const int64_t rows = M - r0 < PLM_HS_CHUNK ? M - r0 : PLM_HS_CHUNK;
    const int rc = plm_gemm_bf16_nt_ws(Y + r0 * ldy, ldy, W, ldw, rest, ld, rows, V, K, 0, 0, nullptr, variant, nullptr, 0, stream);
    if (rc != PLM_OK) return rc;
    const HeadPredictOut o{pred + r0, logp + r0, entropy ? entropy + r0 : nullptr, nll ? nll + r0 : nullptr, lse ? lse + r0 : nullptr};
    plm_launch_head_predict_rows((const uint16_t*)rest, ld, targets ? targets + r0 : nullptr, o, rows, V, s);
  }
  PLM_CHECK_LAUNCH("plm_head_predict_bf16");
  return PLM_OK;
}
