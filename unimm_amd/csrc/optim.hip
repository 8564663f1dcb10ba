// Fused AdamW over the flat fp32 parameter / gradient arenas.
//
// Replaces `pytorch_transformers.AdamW(optimizer_grouped_parameters, lr=...).step()` of the reference
// (train.py:322-347, :458): one group per parameter there, with lr in {lr, image_lr} (config/
// language_weights.json) and weight_decay in {0.01, 0} (bias / LayerNorm).  Published algorithm of that
// class (the library itself is not in this image):
//     m = b1 m + (1-b1) g ;  v = b2 v + (1-b2) g^2 ;  p -= lr sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps) ;
//     p -= lr wd p            (decoupled decay, applied AFTER the Adam update, on the updated value)
// Here the arena is walked once: 16 B per lane, the (lr, wd) group of a 64-element chunk from a byte
// table (arena views are 64-element aligned), the bf16 GEMM-operand copy of the weights written in the
// same pass.  HBM-bound: 4 x 4 B read + 3 x 4 B + 2 B written per parameter.
//
// Optional in front of it (not in the reference, whose train.py does not clip): the global gradient norm in fp64 with a fixed
// summation order, left in a device-resident state block together with the clip coefficient and a non-finite flag, and a second
// instantiation of the step that takes its gradient scale from that block: one more read of g (4 B per parameter), no host sync.
#include "common.h"

namespace {

struct AdamWParams {
  float* p; const float* g; float* m; float* v; bf16_t* w16; const uint8_t* group;
  size_t n;                    // elements (multiple of 4)
  float step_size[UNIMM_ADAMW_MAX_GROUPS];   // lr_g * bias correction
  float decay[UNIMM_ADAMW_MAX_GROUPS];       // lr_g * wd_g
  float beta1, beta2, c1, c2, eps, grad_scale;   // c = 1 - beta, formed in double on the host
  int zero_grad;
};

struct ClipArgs { const unimm_clip_state* st; int skip_nonfinite; };

__device__ __forceinline__ float rnd(float x) { asm volatile("" : "+v"(x)); return x; }

// One body for the plain and the clipped step.  CLIP: the gradient scale is the device word the norm pass left in the state
// block, and a flagged non-finite gradient can turn the whole launch into "clear g and leave".  The plain instantiation is the
// kernel as it was before the switch existed, instruction for instruction: its arguments, its use of a.grad_scale inside the
// loop and the order of the statements it shares with the other are kept for that.
template <bool CLIP, class... Clip>                         // Clip: nothing, or (const unimm_clip_state*, int skip_nonfinite)
__global__ __launch_bounds__(256) void adamw_kernel(AdamWParams a, Clip... clip) {
  __shared__ float s_step[UNIMM_ADAMW_MAX_GROUPS], s_decay[UNIMM_ADAMW_MAX_GROUPS];
  [[maybe_unused]] const unimm_clip_state* st = nullptr;
  if constexpr (CLIP) {
    const auto [st_, skip_nonfinite] = ClipArgs{clip...};
    st = st_;
    if (skip_nonfinite && st->nonfinite) {                   // uniform over the grid: nobody updates
      const size_t nv = a.n >> 2;
      if (a.zero_grad)
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x)
          if (a.group[i >> 4] < UNIMM_ADAMW_MAX_GROUPS)
            reinterpret_cast<f32x4*>(const_cast<float*>(a.g))[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < UNIMM_ADAMW_MAX_GROUPS; ++i)
    if (threadIdx.x == i) { s_step[i] = a.step_size[i]; s_decay[i] = a.decay[i]; }
  __syncthreads();
  const size_t nvec = a.n >> 2;
  const float b1 = a.beta1, b2 = a.beta2, c1 = a.c1, c2 = a.c2;
  [[maybe_unused]] float clip_scale = 0.f;
  if constexpr (CLIP) clip_scale = st->scale;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t gid = a.group[i >> 4];                    // 16 lanes x 4 elements = one 64-element chunk
    if (gid >= UNIMM_ADAMW_MAX_GROUPS) continue;             // parameters that never receive a gradient
    const f32x4 g4 = reinterpret_cast<const f32x4*>(a.g)[i];
    f32x4 p4 = reinterpret_cast<f32x4*>(a.p)[i];
    f32x4 m4 = reinterpret_cast<f32x4*>(a.m)[i];
    f32x4 v4 = reinterpret_cast<f32x4*>(a.v)[i];
    const float ss = s_step[gid], dc = s_decay[gid];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // one rounding per operation, as the reference's separate mul_ / add_ / addcmul_ / addcdiv_ calls have:
      // `rnd` is an empty asm that pins each product in a register so it cannot be contracted into an FMA
      const float g = rnd(g4[e] * (CLIP ? clip_scale : a.grad_scale));
      const float m = rnd(m4[e] * b1) + rnd(c1 * g);
      const float v = rnd(v4[e] * b2) + rnd(rnd(c2 * g) * g);
      const float denom = __fsqrt_rn(v) + a.eps;
      float p = p4[e] + rnd(-ss * rnd(__fdiv_rn(m, denom)));
      if (dc != 0.0f) p = p + rnd(-dc * p);
      m4[e] = m; v4[e] = v; p4[e] = p;
    }
    reinterpret_cast<f32x4*>(a.p)[i] = p4;
    reinterpret_cast<f32x4*>(a.m)[i] = m4;
    reinterpret_cast<f32x4*>(a.v)[i] = v4;
    if (a.w16 != nullptr) reinterpret_cast<u32x2*>(a.w16)[i] = u32x2{pack2bf(p4[0], p4[1]), pack2bf(p4[2], p4[3])};
    if (a.zero_grad) reinterpret_cast<f32x4*>(const_cast<float*>(a.g))[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}


// ---- global gradient norm (include/unimm_hip.h: unimm_grad_norm) ----------------------------------------------------
// HBM-bound like the step: one 16-B load per lane and vector, two vectors in flight per lane and iteration.  Squares and sums
// are fp64 (full rate on this part's vector ALUs: ~70 instructions per 8 elements, a quarter of the time the loads take).
constexpr int NORM_BLOCKS = 2048, NORM_THREADS = 256;      // 8 resident waves per SIMD on 256 CUs
static_assert(NORM_BLOCKS * UNIMM_ADAMW_MAX_GROUPS == UNIMM_GRAD_NORM_WS_DOUBLES, "workspace macro");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double sumsq4(const f32x4 x) {
  const double a = (double)x[0], b = (double)x[1], c = (double)x[2], d = (double)x[3];
  return ((a * a + b * b) + c * c) + d * d;                 // the products are exact in fp64
}
// acc[k] of every lane -> out[k] of the workgroup: butterfly over the wave, then the 4 waves in index order
__device__ __forceinline__ void block_sum8(double (&acc)[UNIMM_ADAMW_MAX_GROUPS], double (*s_part)[UNIMM_ADAMW_MAX_GROUPS],
                                           double* out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < UNIMM_ADAMW_MAX_GROUPS; ++k) {
    const double w = wave_sum_f64(acc[k]);
    if (lane == 0) s_part[wave][k] = w;
  }
  __syncthreads();
  if (threadIdx.x < UNIMM_ADAMW_MAX_GROUPS) {
    const int k = threadIdx.x;
    out[k] = ((s_part[0][k] + s_part[1][k]) + s_part[2][k]) + s_part[3][k];
  }
}

__global__ __launch_bounds__(NORM_THREADS) void grad_sumsq_kernel(const float* __restrict__ g, const uint8_t* __restrict__ group,
                                                                  size_t nvec, uint32_t n_groups, double* __restrict__ ws) {
  __shared__ double s_part[NORM_THREADS / 64][UNIMM_ADAMW_MAX_GROUPS];
  double acc[UNIMM_ADAMW_MAX_GROUPS];
#pragma unroll
  for (int k = 0; k < UNIMM_ADAMW_MAX_GROUPS; ++k) acc[k] = 0.0;
  const size_t T = (size_t)gridDim.x * NORM_THREADS;
  for (size_t i = (size_t)blockIdx.x * NORM_THREADS + threadIdx.x; i < nvec; i += 2 * T) {
    const size_t j = i + T;
    const uint32_t gi = group[i >> 4];                       // 16 lanes x 4 elements = one 64-element chunk
    const uint32_t gj = j < nvec ? (uint32_t)group[j >> 4] : 0xffu;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (gi < n_groups) a = reinterpret_cast<const f32x4*>(g)[i];   // a chunk that does not count is not read: it may hold NaN
    if (gj < n_groups) b = reinterpret_cast<const f32x4*>(g)[j];
    const double sa = sumsq4(a), sb = sumsq4(b);
#pragma unroll
    for (int k = 0; k < UNIMM_ADAMW_MAX_GROUPS; ++k) {       // selects, not a dynamically indexed array (that would live in scratch)
      acc[k] += gi == (uint32_t)k ? sa : 0.0;
      acc[k] += gj == (uint32_t)k ? sb : 0.0;
    }
  }
  block_sum8(acc, s_part, ws + (size_t)blockIdx.x * UNIMM_ADAMW_MAX_GROUPS);
}

__global__ __launch_bounds__(NORM_THREADS) void grad_norm_finish_kernel(const double* __restrict__ ws, int nblocks, int n_groups,
                                                                        float grad_scale, double max_norm, unimm_clip_state* st) {
  __shared__ double s_part[NORM_THREADS / 64][UNIMM_ADAMW_MAX_GROUPS];
  __shared__ double s_tot[UNIMM_ADAMW_MAX_GROUPS];
  double acc[UNIMM_ADAMW_MAX_GROUPS];
#pragma unroll
  for (int k = 0; k < UNIMM_ADAMW_MAX_GROUPS; ++k) acc[k] = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += NORM_THREADS)
#pragma unroll
    for (int k = 0; k < UNIMM_ADAMW_MAX_GROUPS; ++k) acc[k] += ws[(size_t)b * UNIMM_ADAMW_MAX_GROUPS + k];
  block_sum8(acc, s_part, s_tot);
  __syncthreads();
  if (threadIdx.x == 0) {                                    // one lane, plain stores
    double sumsq = 0.0;
    for (int k = 0; k < UNIMM_ADAMW_MAX_GROUPS; ++k) {
      const double t = k < n_groups ? s_tot[k] : 0.0;
      st->group_sumsq[k] = t;
      if (k < n_groups) sumsq += t;
    }
    const int nonfinite = isfinite(sumsq) ? 0 : 1;
    const double norm = fabs((double)grad_scale) * sqrt(sumsq);
    double coef = 1.0;
    if (!nonfinite && max_norm < (double)INFINITY) {
      coef = max_norm / (norm + 1e-6);                       // torch.nn.utils.clip_grad_norm_'s constant
      if (!(coef < 1.0)) coef = 1.0;
    }
    st->sumsq = sumsq; st->norm = norm; st->coef = coef;
    st->scale = (float)((double)grad_scale * coef);
    st->nonfinite = nonfinite;
    st->skipped = st->skipped + nonfinite;
  }
}

}  // namespace

// the checks of unimm_adamw_step and the kernel's parameter block; `blocks`: the grid
static int adamw_prepare(const unimm_adamw_args* a, AdamWParams& p, size_t& blocks) {
  if (a == nullptr || a->p == nullptr || a->g == nullptr || a->m == nullptr || a->v == nullptr || a->group == nullptr)
    return UNIMM_E_ARG;
  if (a->n <= 0 || (a->n % 64) != 0) return UNIMM_E_SHAPE;
  if (((uintptr_t)a->p | (uintptr_t)a->g | (uintptr_t)a->m | (uintptr_t)a->v) & 15) return UNIMM_E_ALIGN;
  if (a->w16 != nullptr && ((uintptr_t)a->w16 & 7)) return UNIMM_E_ALIGN;
  if (a->step < 1 || a->n_groups < 1 || a->n_groups > UNIMM_ADAMW_MAX_GROUPS) return UNIMM_E_ARG;
  p.p = a->p; p.g = a->g; p.m = a->m; p.v = a->v; p.w16 = (bf16_t*)a->w16; p.group = a->group;
  p.n = (size_t)a->n;
  // bias correction in double on the host, as the reference computes it in Python floats
  double corr = 1.0;
  if (a->correct_bias) corr = sqrt(1.0 - pow(a->beta2, (double)a->step)) / (1.0 - pow(a->beta1, (double)a->step));
  for (int i = 0; i < UNIMM_ADAMW_MAX_GROUPS; ++i) {
    const bool on = i < a->n_groups;
    p.step_size[i] = on ? (float)(a->lr[i] * corr) : 0.f;
    p.decay[i] = on ? (float)(a->lr[i] * a->weight_decay[i]) : 0.f;
  }
  p.beta1 = (float)a->beta1; p.beta2 = (float)a->beta2; p.c1 = (float)(1.0 - a->beta1); p.c2 = (float)(1.0 - a->beta2);
  p.eps = (float)a->eps; p.grad_scale = a->grad_scale;
  p.zero_grad = a->zero_grad;
  const size_t nvec = p.n >> 2;
  blocks = (nvec + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;       // grid-stride: 16 workgroups of 4 waves per CU, 8 of them resident at a time (8 waves per SIMD)
  return UNIMM_OK;
}

extern "C" int unimm_adamw_step(const unimm_adamw_args* a, void* stream) {
  AdamWParams p;
  size_t blocks;
  const int rc = adamw_prepare(a, p, blocks);
  if (rc != UNIMM_OK) return rc;
  hipLaunchKernelGGL(adamw_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

extern "C" int unimm_adamw_step_clipped(const unimm_adamw_args* a, const unimm_clip_state* state, int32_t skip_nonfinite,
                                        void* stream) {
  if (state == nullptr) return UNIMM_E_ARG;
  AdamWParams p;
  size_t blocks;
  const int rc = adamw_prepare(a, p, blocks);
  if (rc != UNIMM_OK) return rc;
  if ((uintptr_t)state & 15) return UNIMM_E_ALIGN;
  hipLaunchKernelGGL((adamw_kernel<true, const unimm_clip_state*, int>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, state,
                     (int)(skip_nonfinite != 0));
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

extern "C" int unimm_grad_norm(const float* g, const uint8_t* group, int64_t n, int32_t n_groups, float grad_scale, double max_norm,
                               double* workspace, int64_t workspace_doubles, unimm_clip_state* state, void* stream) {
  if (g == nullptr || group == nullptr || workspace == nullptr || state == nullptr) return UNIMM_E_ARG;
  if (n <= 0 || (n % 64) != 0) return UNIMM_E_SHAPE;
  if (n_groups < 1 || n_groups > UNIMM_ADAMW_MAX_GROUPS) return UNIMM_E_ARG;
  if (!(max_norm > 0.0)) return UNIMM_E_ARG;                 // NaN, zero, negative; +inf = measure only
  if (workspace_doubles < UNIMM_GRAD_NORM_WS_DOUBLES) return UNIMM_E_ARG;
  if (((uintptr_t)g | (uintptr_t)workspace | (uintptr_t)state) & 15) return UNIMM_E_ALIGN;
  const size_t nvec = (size_t)n >> 2;
  size_t blocks = (nvec + 2 * NORM_THREADS - 1) / (2 * NORM_THREADS);   // a function of n alone
  if (blocks > NORM_BLOCKS) blocks = NORM_BLOCKS;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(NORM_THREADS), 0, (hipStream_t)stream, g, group, nvec,
                     (uint32_t)n_groups, workspace);
  UNIMM_CHECK_LAUNCH();
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(NORM_THREADS), 0, (hipStream_t)stream, (const double*)workspace,
                     (int)blocks, (int)n_groups, grad_scale, max_norm, state);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}
