// The optimizer tail (optim/init_optim.py:7-70): AdamW, NAdamW, SGD, signSGD and schedule-free AdamW, each on a flat fp32 span and
// on a list of Linear weights whose bf16 shadows (W and W^T, the operands of the next step's GEMMs) the update writes as well; and
// the lerp that swaps schedule-free parameters between their training (y) and evaluation (x) points.
#include <type_traits>

#include "plm_device.h"
#include "plm_shadow_tile.h"

// torch.lerp's two-sided form (ATen/native/Lerp.h), exact at both ends: a + w (b - a) for |w| < 0.5, else b - (b - a)(1 - w)
__device__ __forceinline__ float lerp_elem(float a, float b, float w) {
  const float d = __fsub_rn(b, a);
  return fabsf(w) < 0.5f ? __fmaf_rn(w, d, a) : __fmaf_rn(-d, __fsub_rn(1.f, w), b);
}

// One element of each update, every rounding spelled out so that the flat kernel and the multi-tensor one give the same bits
// whatever the compiler would contract around them.  __fmul_rn / __fadd_rn are plain operators here and hipcc contracts a product that feeds an addition,
// differently in the two kernels: every product is therefore either a __fmaf_rn operand or the addend of one, never an operand
// of __fadd_rn.  g is pre-multiplied by the clip coefficient, as clip_grad_norm_ does to .grad in place.
template <int KIND>
__device__ __forceinline__ float optim_elem(float p, float g, float& m, float& v, float cs, const plm_optim_hparams& h) {
  const float gi = __fmul_rn(g, cs);
  if constexpr (KIND == PLM_OPTIM_ADAMW) {
    // torch.optim.AdamW, bias corrections folded into the scalars: h is optim_prepared(), so decay = fma(-lr, wd, 1),
    // coef_avg = lr / bc1 and bc2 = sqrt(bc2), each formed in fp32
    const float mi = __fmaf_rn(h.beta1, m, __fmul_rn(1.f - h.beta1, gi));
    const float vi = __fmaf_rn(h.beta2, v, __fmul_rn(__fmul_rn(1.f - h.beta2, gi), gi));
    m = mi;
    v = vi;
    const float d = __fadd_rn(__fdiv_rn(__fsqrt_rn(vi), h.bc2), h.eps);
    return __fmaf_rn(-h.coef_avg, __fdiv_rn(mi, d), __fmul_rn(p, h.decay));
  } else if constexpr (KIND == PLM_OPTIM_NADAMW) {
    // torch.optim.NAdam, decoupled decay: note sqrt(v / bc2), not AdamW's sqrt(v) / sqrt(bc2)
    const float pd = __fmul_rn(p, h.decay);
    const float mi = __fmaf_rn(h.beta1, m, __fmul_rn(1.f - h.beta1, gi));
    const float vi = __fmaf_rn(h.beta2, v, __fmul_rn(__fmul_rn(1.f - h.beta2, gi), gi));
    m = mi;
    v = vi;
    const float d = __fadd_rn(__fsqrt_rn(__fdiv_rn(vi, h.bc2)), h.eps);
    return __fmaf_rn(-h.coef_avg, __fdiv_rn(mi, d), __fmaf_rn(-h.coef_grad, __fdiv_rn(gi, d), pd));
  } else if constexpr (KIND == PLM_OPTIM_SGD) {
    // torch.optim.SGD: coupled L2, the first momentum buffer is the undamped d
    const float d = __fmaf_rn(h.weight_decay, p, gi);
    if (h.momentum == 0.f) return __fmaf_rn(-h.lr, d, p);
    const float mi = h.first ? d : __fmaf_rn(1.f - h.dampening, d, __fmul_rn(h.momentum, m));
    m = mi;
    return __fmaf_rn(-h.lr, mi, p);
  } else if constexpr (KIND == PLM_OPTIM_SFO_ADAMW) {
    // schedule-free AdamW (p = y, m = z, v = exp_avg_sq; `first` creates z as a copy of p and v as zeros), decay at y:
    // gn = g / (sqrt(v / bc2) + eps) + wd y ; y = lerp(y, z, ckp1) + coef_y gn ; z -= lr gn  (the old z in the lerp)
    const float z = h.first ? p : m;
    const float vi = __fmaf_rn(h.beta2, h.first ? 0.f : v, __fmul_rn(__fmul_rn(1.f - h.beta2, gi), gi));
    v = vi;
    const float d = __fadd_rn(__fsqrt_rn(__fdiv_rn(vi, h.bc2)), h.eps);
    const float gn = __fmaf_rn(h.weight_decay, p, __fdiv_rn(gi, d));
    m = __fmaf_rn(-h.lr, gn, z);
    return __fmaf_rn(h.coef_y, gn, lerp_elem(p, z, h.ckp1));
  } else {
    // signSGD: the momentum update runs on the first step too (its first m is (momentum + 1 - dampening) g)
    const float pd = __fmul_rn(p, h.decay);
    const float m0 = h.first ? gi : m;
    const float mi = __fmaf_rn(1.f - h.dampening, gi, __fmul_rn(h.momentum, m0));
    m = mi;
    const float s = mi > 0.f ? 1.f : (mi < 0.f ? -1.f : mi);  // torch.sign: 0 -> 0, NaN -> NaN
    return __fmaf_rn(-h.lr, s, pd);
  }
}

// which state the update reads / writes (block-uniform; compile-time constants for AdamW and NAdamW): the first step of SGD /
// signSGD / schedule-free AdamW does not read the buffers it creates, SGD without momentum has none, SGD and signSGD have no v
template <int KIND>
constexpr bool optim_has_v() { return KIND == PLM_OPTIM_ADAMW || KIND == PLM_OPTIM_NADAMW || KIND == PLM_OPTIM_SFO_ADAMW; }
template <int KIND>
__device__ __forceinline__ bool optim_reads_m(const plm_optim_hparams& h) {
  return KIND == PLM_OPTIM_ADAMW || KIND == PLM_OPTIM_NADAMW || (!h.first && (KIND != PLM_OPTIM_SGD || h.momentum != 0.f));
}
template <int KIND>
__device__ __forceinline__ bool optim_reads_v(const plm_optim_hparams& h) {
  return KIND == PLM_OPTIM_ADAMW || KIND == PLM_OPTIM_NADAMW || (KIND == PLM_OPTIM_SFO_ADAMW && !h.first);
}
template <int KIND>
__device__ __forceinline__ bool optim_writes_m(const plm_optim_hparams& h) {
  return KIND != PLM_OPTIM_SGD || h.momentum != 0.f;
}

// One element per thread, blocks in memory order: measured 29 % faster than a capped grid with a stride loop, and a float4-per-thread
// form of the AdamW kernel 0.94 ms against 0.73 ms for 162 M parameters (profiles/r04_design_notes.md).
template <int KIND>
__global__ __launch_bounds__(256) void optim_kernel(plm_optim_hparams h, float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                    const float* __restrict__ clip) {
  const float cs = clip ? *clip : 1.f;
  const bool rm = optim_reads_m<KIND>(h), wm = optim_writes_m<KIND>(h), rv = optim_reads_v<KIND>(h);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float mi = rm ? m[i] : 0.f;
    float vi = rv ? v[i] : 0.f;
    p[i] = optim_elem<KIND>(p[i], g[i], mi, vi, cs, h);
    if (wm) m[i] = mi;
    if (optim_has_v<KIND>()) v[i] = vi;
  }
}

// The shadow-emitting form: optim_elem on the quads of shadow_tile's walk.  One read of p / g / m / v, one write of p / m / v plus
// 4 bytes per parameter of shadows: the stand-alone cast (one more read of p, the same shadow writes) disappears from the training
// step.  SGD / signSGD move 24 B per parameter, the three Adam kinds 32 B.
struct OptimGroup {
  float* p[PLM_SHADOW_ITEMS_MAX];
  const float* g[PLM_SHADOW_ITEMS_MAX];
  float* m[PLM_SHADOW_ITEMS_MAX];
  float* v[PLM_SHADOW_ITEMS_MAX];
  uint16_t* dst[PLM_SHADOW_ITEMS_MAX];
  uint16_t* dst_t[PLM_SHADOW_ITEMS_MAX];
  ShadowTable shape;
};

template <int KIND>
__global__ __launch_bounds__(256) void optim_cast_multi_kernel(OptimGroup g, plm_optim_hparams h, const float* __restrict__ clip) {
  int64_t r0, c0;
  const int it = shadow_locate(g.shape, r0, c0);
  float* __restrict__ P = g.p[it];
  const float* __restrict__ G = g.g[it];
  float* __restrict__ Mm = g.m[it];
  float* __restrict__ V = g.v[it];
  const float cs = clip ? *clip : 1.f;
  const bool rm = optim_reads_m<KIND>(h), wm = optim_writes_m<KIND>(h), rv = optim_reads_v<KIND>(h);
  shadow_tile(g.dst[it], g.dst_t[it], g.shape.rows[it], g.shape.cols[it], g.shape.ld_t[it], r0, c0, [&](int64_t o) {
    const f32x4_t pv = *reinterpret_cast<const f32x4_t*>(P + o), gv = *reinterpret_cast<const f32x4_t*>(G + o);
    f32x4_t mv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f}, pn;
    if (rm) mv = *reinterpret_cast<const f32x4_t*>(Mm + o);
    if (rv) vv = *reinterpret_cast<const f32x4_t*>(V + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float me = mv[e], ve = vv[e];
      pn[e] = optim_elem<KIND>(pv[e], gv[e], me, ve, cs, h);
      mv[e] = me;
      vv[e] = ve;
    }
    if (wm) *reinterpret_cast<f32x4_t*>(Mm + o) = mv;
    if (optim_has_v<KIND>()) *reinterpret_cast<f32x4_t*>(V + o) = vv;
    *reinterpret_cast<f32x4_t*>(P + o) = pn;
    return pn;
  });
}

static const char* optim_name(int kind) {
  return kind == PLM_OPTIM_ADAMW ? "adamw" : kind == PLM_OPTIM_NADAMW ? "nadamw" : kind == PLM_OPTIM_SGD ? "sgd"
       : kind == PLM_OPTIM_SIGNSGD ? "signSGD" : kind == PLM_OPTIM_SFO_ADAMW ? "sfo_adamw" : nullptr;
}
static bool optim_needs_v(const plm_optim_hparams* h) { return h->kind != PLM_OPTIM_SGD && h->kind != PLM_OPTIM_SIGNSGD; }
static bool optim_needs_m(const plm_optim_hparams* h) { return h->kind != PLM_OPTIM_SGD || h->momentum != 0.f; }

// The struct as the kernels take it.  AdamW's scalars are formed HERE, in fp32 from the fp32 lr / weight_decay / bc1 / bc2, for both
// launch shapes: decay = fma(-lr, wd, 1) (one rounding of the exact product), the step size lr / bc1 in coef_avg, and sqrt(bc2) in
// place of bc2.  The other kinds take decay as the host rounded it from double (include/plainlm_hip.h); the two differ in rare cases
// (lr = 0.826, wd = 0.71: 0.41354004 against 0.41354001), and AdamW's trajectories are pinned bit for bit (tests/golden/adamw_bits.npz).
static plm_optim_hparams optim_prepared(const plm_optim_hparams* h) {
  plm_optim_hparams k = *h;
  if (k.kind == PLM_OPTIM_ADAMW) {
    k.decay = fmaf(-k.lr, k.weight_decay, 1.f);
    k.coef_avg = k.lr / k.bc1;
    k.bc2 = sqrtf(k.bc2);
  }
  return k;
}

// f(std::integral_constant<int, KIND>) for the runtime kind (validated by the caller: optim_name(kind) != nullptr)
template <typename F>
static void optim_dispatch(int kind, F&& f) {
  switch (kind) {
    case PLM_OPTIM_ADAMW: return f(std::integral_constant<int, PLM_OPTIM_ADAMW>());
    case PLM_OPTIM_NADAMW: return f(std::integral_constant<int, PLM_OPTIM_NADAMW>());
    case PLM_OPTIM_SGD: return f(std::integral_constant<int, PLM_OPTIM_SGD>());
    case PLM_OPTIM_SIGNSGD: return f(std::integral_constant<int, PLM_OPTIM_SIGNSGD>());
    default: return f(std::integral_constant<int, PLM_OPTIM_SFO_ADAMW>());
  }
}

extern "C" int plm_optim_f32(const plm_optim_hparams* h, float* p, const float* g, float* m, float* v, int64_t n,
                             const float* clip_coef_dev, void* stream) {
  PLM_REQUIRE(h, "plm_optim_f32: null hparams");
  PLM_REQUIRE(optim_name(h->kind), "plm_optim_f32: unknown optimizer kind %d", h->kind);
  PLM_REQUIRE(p && g && n > 0, "plm_optim_f32: bad arguments");
  PLM_REQUIRE(!optim_needs_m(h) || m, "plm_optim_f32: %s needs the momentum buffer m", optim_name(h->kind));
  PLM_REQUIRE(optim_needs_v(h) == (v != nullptr), "plm_optim_f32: %s %s", optim_name(h->kind),
              optim_needs_v(h) ? "needs v" : "takes no v (pass NULL)");
  const int64_t b = plm_cdiv(n, 256), cap = (int64_t)1 << 20;
  const dim3 grid((unsigned)(b > cap ? cap : b));
  const plm_optim_hparams k = optim_prepared(h);
  optim_dispatch(k.kind, [&](auto kind) {
    hipLaunchKernelGGL(optim_kernel<decltype(kind)::value>, grid, dim3(256), 0, (hipStream_t)stream, k, p, g, m, v, n, clip_coef_dev);
  });
  PLM_CHECK_LAUNCH("plm_optim_f32");
  return PLM_OK;
}

extern "C" int plm_optim_cast_multi(const plm_optim_hparams* h, const plm_optim_item* items, int count, const float* clip_coef_dev,
                                    void* stream) {
  PLM_REQUIRE(h, "plm_optim_cast_multi: null hparams");
  const char* name = optim_name(h->kind);
  PLM_REQUIRE(name, "plm_optim_cast_multi: unknown optimizer kind %d", h->kind);
  const bool need_m = optim_needs_m(h), need_v = optim_needs_v(h);
  const plm_optim_hparams k = optim_prepared(h);
  return shadow_items_run(
      "plm_optim_cast_multi", items, count,
      [&](const plm_optim_item& q, int i) {
        PLM_REQUIRE(q.p && q.g && q.dst && q.dst_t, "plm_optim_cast_multi: null pointer in item %d", i);
        PLM_REQUIRE(!need_m || q.m, "plm_optim_cast_multi: item %d: %s needs the momentum buffer m", i, name);
        PLM_REQUIRE(need_v == (q.v != nullptr), "plm_optim_cast_multi: item %d: %s %s", i, name, need_v ? "needs v" : "takes no v (pass NULL)");
        PLM_REQUIRE(((reinterpret_cast<uintptr_t>(q.p) | reinterpret_cast<uintptr_t>(q.g) | reinterpret_cast<uintptr_t>(q.m) |
                      reinterpret_cast<uintptr_t>(q.v) | reinterpret_cast<uintptr_t>(q.dst) | reinterpret_cast<uintptr_t>(q.dst_t)) & 15) == 0,
                    "plm_optim_cast_multi: item %d: pointers must be 16-byte aligned", i);
        return PLM_OK;
      },
      [&](int first, int n, const ShadowTable& shape) {
        OptimGroup g{};
        for (int i = 0; i < n; ++i) {
          const plm_optim_item& q = items[first + i];
          g.p[i] = q.p; g.g[i] = q.g; g.m[i] = q.m; g.v[i] = q.v; g.dst[i] = q.dst; g.dst_t[i] = q.dst_t;
        }
        g.shape = shape;
        optim_dispatch(k.kind, [&](auto kind) {
          hipLaunchKernelGGL(optim_cast_multi_kernel<decltype(kind)::value>, dim3((unsigned)shape.block_base[n]), dim3(256), 0,
                             (hipStream_t)stream, g, k, clip_coef_dev);
        });
      });
}

// schedule-free train / eval swap: p = lerp(p, z, w) on a flat span (eval: w = 1 - 1/beta1, p = x; train: w = 1 - beta1, p = y)
__global__ __launch_bounds__(256) void lerp_kernel(float* __restrict__ p, const float* __restrict__ z, int64_t n, float w) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = lerp_elem(p[i], z[i], w);
}

extern "C" int plm_lerp_f32(float* p, const float* z, int64_t n, float w, void* stream) {
  PLM_REQUIRE(p && z, "plm_lerp_f32: null p or z");
  PLM_REQUIRE(n > 0, "plm_lerp_f32: n=%ld must be positive", (long)n);
  const int64_t b = plm_cdiv(n, 256), cap = (int64_t)1 << 20;
  hipLaunchKernelGGL(lerp_kernel, dim3((unsigned)(b > cap ? cap : b)), dim3(256), 0, (hipStream_t)stream, p, z, n, w);
  PLM_CHECK_LAUNCH("plm_lerp_f32");
  return PLM_OK;
}
