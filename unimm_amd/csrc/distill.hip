// Token-level knowledge distillation on the decoded rows (gfx950): the student's weighted likelihood / unlikelihood (csrc/loss.hip)
// mixed with the KL from a FROZEN teacher's softened distribution to the student's,
//     rowloss = alpha hard + (1 - alpha) tau^2 KL(softmax(zr / tau) || softmax(z / tau))
// forward and backward (include/unimm_hip.h: unimm_distill_loss_fwd / _bwd).  The layout is that of the likelihood and
// policy-gradient kernels (csrc/loss.hip, csrc/policy.hip): one 256-lane workgroup per row, both fp32 rows read once per direction,
// device-side row count and denominator.  The forward is one pass: a lane keeps, for the student row, the running maximum m,
// s = sum e^(z - m) and st = sum e^((z - m) / tau), and for the teacher row its own maximum mr, sr = sum e^((zr - mr) / tau) and
// ur = sum e^((zr - mr) / tau) (zr - z); then lse = m + log s, lse_t = m / tau + log st, ref_lse_t = mr / tau + log sr and
// KD = ur / (sr tau) - ref_lse_t + lse_t.  The fp32 matrix instruction runs at the vector rate on this chip and the kernels are
// bound by reading two 122 KB rows: there is nothing for MFMA to do here.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, the flags of unimm_amd/build.py):
//   distill_loss_fwd_kernel<true>   56 VGPRs, no scratch, 8 waves per SIMD   (the teacher row is streamed; 65 VGPRs and 7 waves
//                                   without the scheduling fence in row_vector)
//   distill_loss_fwd_kernel<false>  32 VGPRs, no scratch, 8 waves per SIMD   (alpha == 1)
//   distill_loss_bwd_kernel         28 VGPRs, no scratch, 8 waves per SIMD
#include "common.h"

namespace {

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// e^(a - m) and e^((a - m) / tau) (it = 1 / tau); a -inf logit has probability 0 at every temperature and contributes exactly 0
// (never exp(-inf - -inf))
__device__ __forceinline__ float ex(float a, float m) { return a > -INFINITY ? __expf(a - m) : 0.f; }
__device__ __forceinline__ float ext(float a, float m, float it) { return a > -INFINITY ? __expf((a - m) * it) : 0.f; }
// the share of ur = sum e^((zr - mr) / tau) (zr - z) of one column: 0 where the teacher's logit is -inf, whatever the student
// holds there (never 0 * inf, never -inf - -inf)
__device__ __forceinline__ float eu(float q, float r, float a) { return r > -INFINITY ? q * (r - a) : 0.f; }

// four consecutive floats of a row: one 16-byte load when the row's stride keeps them aligned, four scalar loads otherwise
template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* __restrict__ p) {
  if (VEC) return *reinterpret_cast<const f32x4*>(p);
  return f32x4{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ float max4(const f32x4& a) { return fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])); }

// running state of a lane: the student row's (m, s, st) and, with the soft term, the teacher row's own (mr, sr, ur)
struct RowAcc {
  float m = -INFINITY, s = 0.f, st = 0.f, mr = -INFINITY, sr = 0.f, ur = 0.f;
};
// a new running maximum: the sums are rescaled to it.  (m, s) take csrc/loss.hip's row_lse operations; (mr, sr) take (m, st)'s.
__device__ __forceinline__ void raise(RowAcc& c, float mm, float it) {
  if (mm > c.m) { const float d = c.m - mm; c.s *= __expf(d); c.st *= __expf(d * it); c.m = mm; }
}
__device__ __forceinline__ void raise_ref(RowAcc& c, float mq, float it) {
  if (mq > c.mr) { const float f = __expf((c.mr - mq) * it); c.sr *= f; c.ur *= f; c.mr = mq; }
}

// columns i, i + 256, ... < V one at a time
template <bool SOFT>
__device__ __forceinline__ void row_scalar(const float* __restrict__ z, const float* __restrict__ zr, int i, int V, float it,
                                           RowAcc& c) {
  for (; i < V; i += 256) {
    const float a = z[i];
    raise(c, a, it);
    c.s += ex(a, c.m);
    c.st += ext(a, c.m, it);
    if (SOFT) {
      const float r = zr[i];
      raise_ref(c, r, it);
      const float q = ext(r, c.mr, it);
      c.sr += q;
      c.ur += eu(q, r, a);
    }
  }
}

// the first nv float4 groups of the row with 16-byte loads of the student row (and of the teacher row when RV)
template <bool SOFT, bool RV>
__device__ __forceinline__ void row_vector(const float* __restrict__ z, const float* __restrict__ zr, int nv, float it, RowAcc& c) {
  int i = threadIdx.x;
  for (; i + 768 < nv; i += 1024) {        // four 16-byte loads in flight per lane and row (a row is read once, from HBM)
    f32x4 a[4], r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = *reinterpret_cast<const f32x4*>(z + 4 * (i + 256 * u));
    if (SOFT) {
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = load4<RV>(zr + 4 * (i + 256 * u));
    }
    float mm = -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u) mm = fmaxf(mm, max4(a[u]));
    raise(c, mm, it);
    if (SOFT) {                            // the teacher row's log-sum-exp: the student row's operations, on its own state
      float mq = -INFINITY;
#pragma unroll
      for (int u = 0; u < 4; ++u) mq = fmaxf(mq, max4(r[u]));
      raise_ref(c, mq, it);
    }
    float mu = c.m, mq = c.mr;
#pragma unroll
    for (int u = 0; u < 4; ++u) {          // (both rows' group u is consumed here: its eight registers are free afterwards)
      // A group's exponentials wait for the previous group's sums (an empty statement the compiler cannot look through; the
      // values are unchanged), as in csrc/policy.hip's pair with a reference: scheduled freely, the exponentials of several
      // groups are hoisted above their use and the kernel takes 65 VGPRs, 7 waves per SIMD instead of 8.
      if (SOFT) asm volatile("" : "+v"(mu), "+v"(mq) : "v"(c.s), "v"(c.st), "v"(c.sr), "v"(c.ur));
      c.s += ex(a[u][0], mu) + ex(a[u][1], mu) + ex(a[u][2], mu) + ex(a[u][3], mu);
      c.st += ext(a[u][0], mu, it) + ext(a[u][1], mu, it) + ext(a[u][2], mu, it) + ext(a[u][3], mu, it);
      if (SOFT) {
        const float q0 = ext(r[u][0], mq, it), q1 = ext(r[u][1], mq, it), q2 = ext(r[u][2], mq, it), q3 = ext(r[u][3], mq, it);
        c.sr += q0 + q1 + q2 + q3;
        c.ur += eu(q0, r[u][0], a[u][0]) + eu(q1, r[u][1], a[u][1]) + eu(q2, r[u][2], a[u][2]) + eu(q3, r[u][3], a[u][3]);
      }
    }
  }
  for (; i < nv; i += 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(z + 4 * i);
    raise(c, max4(a), it);
    c.s += ex(a[0], c.m) + ex(a[1], c.m) + ex(a[2], c.m) + ex(a[3], c.m);
    c.st += ext(a[0], c.m, it) + ext(a[1], c.m, it) + ext(a[2], c.m, it) + ext(a[3], c.m, it);
    if (SOFT) {
      const f32x4 r = load4<RV>(zr + 4 * i);
      raise_ref(c, max4(r), it);
      const float q0 = ext(r[0], c.mr, it), q1 = ext(r[1], c.mr, it), q2 = ext(r[2], c.mr, it), q3 = ext(r[3], c.mr, it);
      c.sr += q0 + q1 + q2 + q3;
      c.ur += eu(q0, r[0], a[0]) + eu(q1, r[1], a[1]) + eu(q2, r[2], a[2]) + eu(q3, r[3], a[3]);
    }
  }
}

// The row's three log-sum-exps and KD in one read of both rows (16-byte loads of the student row when `vec`), block-wide.  m and s
// take the values of csrc/loss.hip's row_lse operation for operation (rownll and lse are unimm_lm_loss_fwd's bit for bit: keep
// the two in step; a -inf logit is guarded here as in csrc/policy.hip, which changes no value row_lse defines); st rides along with
// tau = 1 giving st == s.  SOFT: the teacher row zr is read beside it, column for column in the student row's order (so its
// 16-byte loads need `rvec` AND `vec`: with a student row on the scalar path both rows are read one column at a time); its
// (mr, sr) take the operation sequence of the student's (m, st): zr == z gives ref_lse_t == lse_t bitwise and kd == +0.
template <bool SOFT>
__device__ __forceinline__ void row_stats(const float* __restrict__ z, const float* __restrict__ zr, int V, bool vec, bool rvec,
                                          float tau, float it, float* red, float& lse, float& lse_t, float& ref_lse_t, float& kd) {
  RowAcc c;
  if (vec) {
    const int nv = V >> 2;
    if (!SOFT || rvec) row_vector<SOFT, true>(z, zr, nv, it, c);
    else row_vector<SOFT, false>(z, zr, nv, it, c);
    row_scalar<SOFT>(z, zr, (nv << 2) + threadIdx.x, V, it, c);
  } else {
    row_scalar<SOFT>(z, zr, threadIdx.x, V, it, c);
  }
  const float gm = block_max(c.m, red);
  const float gs = block_sum(c.m == -INFINITY ? 0.f : c.s * __expf(c.m - gm), red);
  const float gst = block_sum(c.m == -INFINITY ? 0.f : c.st * __expf((c.m - gm) * it), red);
  lse = gm + logf(gs);
  lse_t = fmaf(gm, it, logf(gst));
  if (SOFT) {
    const float gmr = block_max(c.mr, red);
    const float fr = c.mr == -INFINITY ? 0.f : __expf((c.mr - gmr) * it);
    const float gsr = block_sum(c.mr == -INFINITY ? 0.f : c.sr * fr, red);
    const float gur = block_sum(c.mr == -INFINITY ? 0.f : c.ur * fr, red);
    ref_lse_t = fmaf(gmr, it, logf(gsr));
    kd = gur / (gsr * tau) - ref_lse_t + lse_t;
  }
}

// whether a row takes part: a label and a weight the likelihood kernels give a loss for
__device__ __forceinline__ bool takes_part(int y, int w) { return y >= 0 && (w > 0 || w == -1); }

// SOFT = false: alpha == 1, the teacher row is not read (ref_lse_t and kd are written as 0)
template <bool SOFT>
__global__ __launch_bounds__(256) void distill_loss_fwd_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                               const int32_t* __restrict__ weights,
                                                               const float* __restrict__ ref_logits, int ld_ref, float tau,
                                                               float alpha, float* __restrict__ rowloss, float* __restrict__ rownll,
                                                               float* __restrict__ lse_o, float* __restrict__ lse_t_o,
                                                               float* __restrict__ ref_lse_t_o, float* __restrict__ kd_o, int V,
                                                               int ld, float clamp_min, const int32_t* __restrict__ n_dev) {
  __shared__ float red[4];
  const int row = blockIdx.x;
  if (n_dev != nullptr && row >= n_dev[0]) return;      // rows of the launch's capacity beyond the step's real count
  const float* z = logits + (size_t)row * ld;
  const float* zr = SOFT ? ref_logits + (size_t)row * ld_ref : nullptr;
  const float it = 1.0f / tau;
  float lse, lse_t, ref_lse_t = 0.f, kd = 0.f;
  row_stats<SOFT>(z, zr, V, (ld & 3) == 0, SOFT && (ld_ref & 3) == 0, tau, it, red, lse, lse_t, ref_lse_t, kd);
  if (threadIdx.x == 0) {
    const int y = labels[row], w = weights[row];
    float loss = 0.f, nll = 0.f;                         // the hard term: unimm_lm_loss_fwd's statements
    if (y >= 0) {
      const float logp = z[y] - lse;
      nll = -logp;
      if (w > 0) loss = -logp * (float)w;
      else if (w == -1) loss = -logf(fmaxf(1.0f - expf(logp), clamp_min));
    }
    const bool part = takes_part(y, w);
    // (SOFT = false: alpha == 1, the hard term's bits; alpha == 0: the hard term is not added -- it is +inf on a -inf label)
    if (SOFT && part) loss = (alpha != 0.f ? alpha * loss : 0.f) + ((1.0f - alpha) * tau * tau) * kd;
    rowloss[row] = loss;
    rownll[row] = nll;
    lse_o[row] = lse;
    lse_t_o[row] = lse_t;
    ref_lse_t_o[row] = ref_lse_t;
    kd_o[row] = part ? kd : 0.f;
  }
}

// a softened probability e^(v / tau - l): the same expression for both rows, so that a teacher row equal to the student's (and
// ref_lse_t == lse_t) gives a difference of exactly zero; v = -inf gives 0
__device__ __forceinline__ float soft_p(float v, float it, float l) { return __expf(fmaf(v, it, -l)); }

// dlogits = g inv (alpha hard' + (1 - alpha) tau (e^(z_i / tau - lse_t) - e^(zr_i / tau - ref_lse_t))); hard' is
// unimm_lm_loss_bwd's element, statement for statement.  Each of the two rows takes 16-byte loads when its own stride allows.
__global__ __launch_bounds__(256) void distill_loss_bwd_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                               const int32_t* __restrict__ weights,
                                                               const float* __restrict__ ref_logits, int ld_ref, float tau,
                                                               float alpha, const float* __restrict__ lse_i,
                                                               const float* __restrict__ lse_t_i, const float* __restrict__ ref_lse_t_i,
                                                               const float* __restrict__ g, float inv_denom,
                                                               bf16_t* __restrict__ dlogits, int V, int ld, int ldd, float clamp_min,
                                                               const int32_t* __restrict__ n_dev, const float* __restrict__ inv_dev) {
  const int row = blockIdx.x;
  if (n_dev != nullptr && row >= n_dev[0]) return;
  if (inv_dev != nullptr) inv_denom = inv_dev[0];
  const float* z = logits + (size_t)row * ld;
  bf16_t* dz = dlogits + (size_t)row * ldd;
  const int y = labels[row], w = weights[row];
  const float lse = lse_i[row];
  float coef = 0.f, cs = 0.f;
  if (y >= 0) {
    const float gs = g[0] * inv_denom;
    if (w > 0) coef = gs * (float)w;
    else if (w == -1) {
      const float py = expf(z[y] - lse);
      const float om = 1.0f - py;
      coef = om >= clamp_min ? -gs * py / om : 0.f;   // d/dz of -log(clamp(1-p_y)): zero once clamped
    }
    coef *= alpha;                                    // (alpha == 1: unimm_lm_loss_bwd's coefficient, bit for bit)
    if (alpha != 1.0f && takes_part(y, w)) cs = gs * ((1.0f - alpha) * tau);
  }
  const int n8 = ldd >> 3;
  if (coef == 0.f && cs == 0.f) {                     // a row that takes no part, or whose terms are both off: zeros, no logit is read
    for (int i = threadIdx.x; i < n8; i += 256) *reinterpret_cast<u32x4*>(dz + 8 * i) = u32x4{0u, 0u, 0u, 0u};
    return;
  }
  // 8 columns per lane and iteration: two 16-byte loads per row, one 16-byte store (ldd % 8 == 0; columns >= V are written as
  // zeros: K padding of the dgrad GEMM).  A row is 16-byte aligned when its stride is a multiple of 4 floats.
  const bool with_hard = coef != 0.f, with_soft = cs != 0.f;
  const bool vec = (ld & 3) == 0, rvec = (ld_ref & 3) == 0;
  const float* zr = with_soft ? ref_logits + (size_t)row * ld_ref : nullptr;
  const float it = 1.0f / tau;
  const float lse_t = with_soft ? lse_t_i[row] : 0.f, rlse_t = with_soft ? ref_lse_t_i[row] : 0.f;
  for (int i = threadIdx.x; i < n8; i += 256) {
    const int c0 = 8 * i;
    float v[8], q[8];
    const bool full = c0 + 8 <= V;
    if (vec && full) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(z + c0), b2 = *reinterpret_cast<const f32x4*>(z + c0 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b2[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (c0 + e < V) ? z[c0 + e] : -INFINITY;
    }
    if (with_soft) {                                  // the teacher row's columns (never past V)
      if (rvec && full) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(zr + c0), b2 = *reinterpret_cast<const f32x4*>(zr + c0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { q[e] = a[e]; q[4 + e] = b2[e]; }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = (c0 + e < V) ? zr[c0 + e] : -INFINITY;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + e;
      float d = with_hard ? coef * (__expf(v[e] - lse) - (c == y ? 1.0f : 0.0f)) : 0.f;
      if (with_soft) d += cs * (soft_p(v[e], it, lse_t) - soft_p(q[e], it, rlse_t));
      v[e] = (full || c < V) ? d : 0.f;
    }
    *reinterpret_cast<u32x4*>(dz + c0) = u32x4{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
  }
}

// temperature finite and > 0, hard-label share in [0, 1]; the teacher's rows at least V wide wherever they are read
int distill_args_bad(const float* ref_logits, int ld_ref, int V, float tau, float alpha) {
  if (!(tau > 0.f) || !(tau < INFINITY) || !(alpha >= 0.f) || !(alpha <= 1.f)) return 1;
  if (alpha != 1.0f && !ref_logits) return 1;
  return ref_logits != nullptr && ld_ref < V;
}

}  // namespace

extern "C" int unimm_distill_loss_fwd(const float* logits, const int32_t* labels, const int32_t* weights, const float* ref_logits,
                                      int32_t ld_ref, float tau, float alpha, float* rowloss, float* rownll, float* lse,
                                      float* lse_t, float* ref_lse_t, float* kd, int32_t n, int32_t V, int32_t ld,
                                      const int32_t* n_dev, void* stream) {
  if (!logits || !labels || !weights || !rowloss || !rownll || !lse || !lse_t || !ref_lse_t || !kd) return UNIMM_E_ARG;
  if (distill_args_bad(ref_logits, ld_ref, V, tau, alpha)) return UNIMM_E_ARG;
  if (n <= 0 || V <= 0 || V > 65536 || ld < V) return UNIMM_E_SHAPE;
  if (alpha != 1.0f)
    hipLaunchKernelGGL(distill_loss_fwd_kernel<true>, dim3(n), dim3(256), 0, (hipStream_t)stream, logits, labels, weights, ref_logits,
                       ld_ref, tau, alpha, rowloss, rownll, lse, lse_t, ref_lse_t, kd, V, ld, 1e-6f, n_dev);
  else
    hipLaunchKernelGGL(distill_loss_fwd_kernel<false>, dim3(n), dim3(256), 0, (hipStream_t)stream, logits, labels, weights, nullptr,
                       0, tau, alpha, rowloss, rownll, lse, lse_t, ref_lse_t, kd, V, ld, 1e-6f, n_dev);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

extern "C" int unimm_distill_loss_bwd(const float* logits, const int32_t* labels, const int32_t* weights, const float* ref_logits,
                                      int32_t ld_ref, float tau, float alpha, const float* lse, const float* lse_t,
                                      const float* ref_lse_t, const float* g, float inv_denom, void* dlogits, int32_t n, int32_t V,
                                      int32_t ld, int32_t ldd, const int32_t* n_dev, const float* inv_dev, void* stream) {
  if (!logits || !labels || !weights || !lse || !lse_t || !ref_lse_t || !g || !dlogits) return UNIMM_E_ARG;
  if (distill_args_bad(ref_logits, ld_ref, V, tau, alpha)) return UNIMM_E_ARG;
  if (n <= 0 || V <= 0 || V > 65536 || ld < V || ldd < V || (ldd % 8)) return UNIMM_E_SHAPE;
  hipLaunchKernelGGL(distill_loss_bwd_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, logits, labels, weights, ref_logits, ld_ref,
                     tau, alpha, lse, lse_t, ref_lse_t, g, inv_denom, (bf16_t*)dlogits, V, ld, ldd, 1e-6f, n_dev, inv_dev);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}
