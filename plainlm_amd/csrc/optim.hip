// The reference's other optimizer tails (optim/init_optim.py:7-70): NAdamW, SGD, signSGD and schedule-free AdamW on the flat fp32
// spans and on the shadow-emitting Linear-weight lists, the two launch shapes of the AdamW tail in elementwise.hip; and the lerp that
// swaps schedule-free parameters between their training (y) and evaluation (x) points.
#include "plm_device.h"

// torch.lerp's two-sided form (ATen/native/Lerp.h), exact at both ends: a + w (b - a) for |w| < 0.5, else b - (b - a)(1 - w)
__device__ __forceinline__ float lerp_elem(float a, float b, float w) {
  const float d = __fsub_rn(b, a);
  return fabsf(w) < 0.5f ? __fmaf_rn(w, d, a) : __fmaf_rn(-d, __fsub_rn(1.f, w), b);
}

// One element of each update, every rounding spelled out (as adamw_elem does) so that the flat kernel and the multi-tensor
// one give the same bits.  __fmul_rn / __fadd_rn are plain operators here and hipcc contracts a product that feeds an addition,
// differently in the two kernels: every product is therefore either a __fmaf_rn operand or the addend of one, never an operand
// of __fadd_rn.  g is pre-multiplied by the clip coefficient, as clip_grad_norm_ does to .grad in place.
template <int KIND>
__device__ __forceinline__ float optim_elem(float p, float g, float& m, float& v, float cs, const plm_optim_hparams& h) {
  const float gi = __fmul_rn(g, cs);
  if constexpr (KIND == PLM_OPTIM_NADAMW) {
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

// which state the update reads / writes (block-uniform): the first step of SGD / signSGD / schedule-free AdamW does not read the
// buffers it creates, SGD without momentum has none, only NAdamW and schedule-free AdamW have v
template <int KIND>
__device__ __forceinline__ bool optim_reads_m(const plm_optim_hparams& h) {
  return KIND == PLM_OPTIM_NADAMW || (!h.first && (KIND != PLM_OPTIM_SGD || h.momentum != 0.f));
}
template <int KIND>
__device__ __forceinline__ bool optim_reads_v(const plm_optim_hparams& h) {
  return KIND == PLM_OPTIM_NADAMW || (KIND == PLM_OPTIM_SFO_ADAMW && !h.first);
}
template <int KIND>
constexpr bool optim_has_v() { return KIND == PLM_OPTIM_NADAMW || KIND == PLM_OPTIM_SFO_ADAMW; }
template <int KIND>
__device__ __forceinline__ bool optim_writes_m(const plm_optim_hparams& h) {
  return KIND != PLM_OPTIM_SGD || h.momentum != 0.f;
}

// one element per thread, blocks in memory order (the layout adamw_kernel measured fastest)
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

// The shadow-emitting form: the 64 x 64 tile walk, LDS transposition and block_base search of adamw_cast_multi_kernel, with
// optim_elem per element.  SGD / signSGD move 24 B per parameter (p, g, m read; p, m written; 4 B of shadows), NAdamW and
// schedule-free AdamW 32 B.
#define PLM_OPTIM_MULTI_MAX 56
struct OptimGroup {
  float* p[PLM_OPTIM_MULTI_MAX];
  const float* g[PLM_OPTIM_MULTI_MAX];
  float* m[PLM_OPTIM_MULTI_MAX];
  float* v[PLM_OPTIM_MULTI_MAX];
  uint16_t* dst[PLM_OPTIM_MULTI_MAX];
  uint16_t* dst_t[PLM_OPTIM_MULTI_MAX];
  int rows[PLM_OPTIM_MULTI_MAX], cols[PLM_OPTIM_MULTI_MAX], ld_t[PLM_OPTIM_MULTI_MAX];
  int block_base[PLM_OPTIM_MULTI_MAX + 1];
  int count;
};

template <int KIND>
__global__ __launch_bounds__(256) void optim_cast_multi_kernel(OptimGroup g, plm_optim_hparams h, const float* __restrict__ clip) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[64][72];
  int it = 0;
  for (int q = 1; q < g.count; ++q)
    if ((int)blockIdx.x >= g.block_base[q]) it = q;  // block-uniform scalar search
  const int local = blockIdx.x - g.block_base[it];
  const int tiles_x = (g.cols[it] + 63) / 64;
  const int64_t rows = g.rows[it], cols = g.cols[it], ld_t = g.ld_t[it];
  float* __restrict__ P = g.p[it];
  const float* __restrict__ G = g.g[it];
  float* __restrict__ Mm = g.m[it];
  float* __restrict__ V = g.v[it];
  uint16_t* __restrict__ dst = g.dst[it];
  uint16_t* __restrict__ dst_t = g.dst_t[it];
  const int64_t r0 = (int64_t)(local / tiles_x) * 64, c0 = (int64_t)(local % tiles_x) * 64;
  const float cs = clip ? *clip : 1.f;
  const bool rm = optim_reads_m<KIND>(h), wm = optim_writes_m<KIND>(h), rv = optim_reads_v<KIND>(h);
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (t >> 4) + 16 * i, c = (t & 15) * 4;
    const int64_t gr = r0 + r, gc = c0 + c;
    const bool in = gr < rows && gc < cols;  // cols % 8 == 0: the four columns are in range together
    f32x4_t pn = {0.f, 0.f, 0.f, 0.f};
    if (in) {
      const int64_t o = gr * cols + gc;
      const f32x4_t pv = *reinterpret_cast<const f32x4_t*>(P + o), gv = *reinterpret_cast<const f32x4_t*>(G + o);
      f32x4_t mv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
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
    }
    bf16x4_t o4;
    o4[0] = f2bf(pn[0]); o4[1] = f2bf(pn[1]); o4[2] = f2bf(pn[2]); o4[3] = f2bf(pn[3]);
    if (in) st_bf16x4(dst + gr * cols + gc, o4);
    tile[c + 0][r] = o4[0]; tile[c + 1][r] = o4[1]; tile[c + 2][r] = o4[2]; tile[c + 3][r] = o4[3];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = (t >> 3) + 32 * i, rch = (t & 7) * 8;
    const int64_t gc = c0 + c, gr = r0 + rch;
    if (gc < cols && gr < rows) {
      const bf16x8_t v8 = *reinterpret_cast<const bf16x8_t*>(&tile[c][rch]);
      st_bf16x8(dst_t + gc * ld_t + gr, v8);
    }
  }
}

static const char* optim_name(int kind) {
  return kind == PLM_OPTIM_NADAMW ? "nadamw" : kind == PLM_OPTIM_SGD ? "sgd" : kind == PLM_OPTIM_SIGNSGD ? "signSGD"
       : kind == PLM_OPTIM_SFO_ADAMW ? "sfo_adamw" : nullptr;
}
static bool optim_needs_v(const plm_optim_hparams* h) { return h->kind == PLM_OPTIM_NADAMW || h->kind == PLM_OPTIM_SFO_ADAMW; }
static bool optim_needs_m(const plm_optim_hparams* h) { return h->kind != PLM_OPTIM_SGD || h->momentum != 0.f; }

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
  if (h->kind == PLM_OPTIM_NADAMW)
    hipLaunchKernelGGL(optim_kernel<PLM_OPTIM_NADAMW>, grid, dim3(256), 0, (hipStream_t)stream, *h, p, g, m, v, n, clip_coef_dev);
  else if (h->kind == PLM_OPTIM_SFO_ADAMW)
    hipLaunchKernelGGL(optim_kernel<PLM_OPTIM_SFO_ADAMW>, grid, dim3(256), 0, (hipStream_t)stream, *h, p, g, m, v, n, clip_coef_dev);
  else if (h->kind == PLM_OPTIM_SGD)
    hipLaunchKernelGGL(optim_kernel<PLM_OPTIM_SGD>, grid, dim3(256), 0, (hipStream_t)stream, *h, p, g, m, v, n, clip_coef_dev);
  else
    hipLaunchKernelGGL(optim_kernel<PLM_OPTIM_SIGNSGD>, grid, dim3(256), 0, (hipStream_t)stream, *h, p, g, m, v, n, clip_coef_dev);
  PLM_CHECK_LAUNCH("plm_optim_f32");
  return PLM_OK;
}

extern "C" int plm_optim_cast_multi(const plm_optim_hparams* h, const plm_adamw_item* items, int count, const float* clip_coef_dev,
                                    void* stream) {
  PLM_REQUIRE(h, "plm_optim_cast_multi: null hparams");
  const char* name = optim_name(h->kind);
  PLM_REQUIRE(name, "plm_optim_cast_multi: unknown optimizer kind %d", h->kind);
  PLM_REQUIRE(items && count >= 1, "plm_optim_cast_multi: null pointer or empty list");
  const bool need_m = optim_needs_m(h), need_v = optim_needs_v(h);
  int64_t tiles = 0;
  // validate every item before the first launch: a refused list leaves all parameters as they were
  for (int i = 0; i < count; ++i) {
    const plm_adamw_item& q = items[i];
    PLM_REQUIRE(q.p && q.g && q.dst && q.dst_t, "plm_optim_cast_multi: null pointer in item %d", i);
    PLM_REQUIRE(!need_m || q.m, "plm_optim_cast_multi: item %d: %s needs the momentum buffer m", i, name);
    PLM_REQUIRE(need_v == (q.v != nullptr), "plm_optim_cast_multi: item %d: %s %s", i, name, need_v ? "needs v" : "takes no v (pass NULL)");
    PLM_REQUIRE(q.rows > 0 && q.cols > 0 && q.rows % 8 == 0 && q.cols % 8 == 0 && q.rows < (1ll << 31) && q.cols < (1ll << 31),
                "plm_optim_cast_multi: item %d: rows=%ld cols=%ld must be positive multiples of 8", i, (long)q.rows, (long)q.cols);
    PLM_REQUIRE(q.ld_t >= q.rows && q.ld_t % 8 == 0 && q.ld_t < (1ll << 31),
                "plm_optim_cast_multi: item %d: ld_t=%ld must be >= rows and a multiple of 8", i, (long)q.ld_t);
    PLM_REQUIRE(((reinterpret_cast<uintptr_t>(q.p) | reinterpret_cast<uintptr_t>(q.g) | reinterpret_cast<uintptr_t>(q.m) |
                  reinterpret_cast<uintptr_t>(q.v) | reinterpret_cast<uintptr_t>(q.dst) | reinterpret_cast<uintptr_t>(q.dst_t)) & 15) == 0,
                "plm_optim_cast_multi: item %d: pointers must be 16-byte aligned", i);
    tiles += plm_cdiv(q.rows, 64) * plm_cdiv(q.cols, 64);
    PLM_REQUIRE(tiles < (1ll << 31), "plm_optim_cast_multi: too many tiles");
  }
  for (int first = 0; first < count; first += PLM_OPTIM_MULTI_MAX) {
    const int n = count - first < PLM_OPTIM_MULTI_MAX ? count - first : PLM_OPTIM_MULTI_MAX;
    OptimGroup g{};
    int64_t base = 0;
    for (int i = 0; i < n; ++i) {
      const plm_adamw_item& q = items[first + i];
      g.p[i] = q.p; g.g[i] = q.g; g.m[i] = q.m; g.v[i] = q.v; g.dst[i] = q.dst; g.dst_t[i] = q.dst_t;
      g.rows[i] = (int)q.rows; g.cols[i] = (int)q.cols; g.ld_t[i] = (int)q.ld_t;
      g.block_base[i] = (int)base;
      base += plm_cdiv(q.rows, 64) * plm_cdiv(q.cols, 64);
    }
    g.block_base[n] = (int)base;
    g.count = n;
    if (h->kind == PLM_OPTIM_NADAMW)
      hipLaunchKernelGGL(optim_cast_multi_kernel<PLM_OPTIM_NADAMW>, dim3((unsigned)base), dim3(256), 0, (hipStream_t)stream, g, *h, clip_coef_dev);
    else if (h->kind == PLM_OPTIM_SFO_ADAMW)
      hipLaunchKernelGGL(optim_cast_multi_kernel<PLM_OPTIM_SFO_ADAMW>, dim3((unsigned)base), dim3(256), 0, (hipStream_t)stream, g, *h, clip_coef_dev);
    else if (h->kind == PLM_OPTIM_SGD)
      hipLaunchKernelGGL(optim_cast_multi_kernel<PLM_OPTIM_SGD>, dim3((unsigned)base), dim3(256), 0, (hipStream_t)stream, g, *h, clip_coef_dev);
    else
      hipLaunchKernelGGL(optim_cast_multi_kernel<PLM_OPTIM_SIGNSGD>, dim3((unsigned)base), dim3(256), 0, (hipStream_t)stream, g, *h, clip_coef_dev);
    PLM_CHECK_LAUNCH("plm_optim_cast_multi");
  }
  return PLM_OK;
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
