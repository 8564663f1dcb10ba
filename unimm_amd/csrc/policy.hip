// Policy-gradient objective on the decoded rows of sampled answers (gfx950): REINFORCE / self-critical (A log p_y), the
// clipped importance-weighted surrogate (min(r A, clamp(r, 1-eps, 1+eps) A), r = p_y / q_y) and an entropy bonus -- forward and
// backward.  The layout is that of the likelihood kernels (csrc/loss.hip): one 256-lane workgroup per row, fp32 logits read
// once per direction, device-side row count and denominator.  The row's entropy comes out of the SAME pass as its
// log-sum-exp: next to the running maximum m and s = sum e^(z-m) a lane keeps t = sum e^(z-m) z, rescaled with s, and
// H = -sum p log p = lse - t / s.
// The KL-regularised pair (unimm_pg_kl_loss_*) streams a frozen reference's row beside the policy's in the same pass: a lane
// also keeps u = sum e^(z-m) (z - zr) and the reference row's own (mr, sr), and KL(p || pr) = u / s - lse + ref_lse.  Both
// pairs are instantiations of one template, so the policy row's m, s, t are computed by the same source either way.
#include "common.h"

namespace {

enum { PG_LOGP = 0, PG_RATIO = 1 };

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

// e^(a-m) and its share of t; a -inf logit has probability 0 and contributes exactly 0 to both (never exp(-inf - -inf), never
// 0 * inf)
__device__ __forceinline__ float ex(float a, float m) { return a > -INFINITY ? __expf(a - m) : 0.f; }
__device__ __forceinline__ float ez(float e, float a) { return a > -INFINITY ? e * a : 0.f; }

// the share of u = sum e^(z-m) (z - zr) of one column: 0 where the policy's logit is -inf, whatever the reference holds there
__device__ __forceinline__ float eu(float e, float a, float r) { return a > -INFINITY ? e * (a - r) : 0.f; }

// four consecutive floats of a row: one 16-byte load when the row's stride keeps them aligned, four scalar loads otherwise
template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* __restrict__ p) {
  if (VEC) return *reinterpret_cast<const f32x4*>(p);
  return f32x4{p[0], p[1], p[2], p[3]};
}

// running state of a lane: the policy row's (m, s, t) and, with KL, u and the reference row's own (mr, sr)
struct RowAcc {
  float m = -INFINITY, s = 0.f, t = 0.f, u = 0.f, mr = -INFINITY, sr = 0.f;
};

// columns i, i + 256, ... < V one at a time
template <bool KL>
__device__ __forceinline__ void row_scalar(const float* __restrict__ z, const float* __restrict__ zr, int i, int V, RowAcc& c) {
  for (; i < V; i += 256) {
    const float a = z[i];
    if (a > c.m) { const float f = __expf(c.m - a); c.s *= f; c.t *= f; if (KL) c.u *= f; c.m = a; }
    const float e = ex(a, c.m);
    c.s += e;
    c.t += ez(e, a);
    if (KL) {
      const float r = zr[i];
      c.u += eu(e, a, r);
      if (r > c.mr) { const float f = __expf(c.mr - r); c.sr *= f; c.mr = r; }
      c.sr += ex(r, c.mr);
    }
  }
}

// the first nv float4 groups of the row with 16-byte loads of the policy row (and of the reference row when RV)
template <bool KL, bool RV>
__device__ __forceinline__ void row_vector(const float* __restrict__ z, const float* __restrict__ zr, int nv, RowAcc& c) {
  int i = threadIdx.x;
  for (; i + 768 < nv; i += 1024) {        // four 16-byte loads in flight per lane and row (a row is read once, from HBM)
    f32x4 a[4], r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = *reinterpret_cast<const f32x4*>(z + 4 * (i + 256 * u));
    if (KL) {
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = load4<RV>(zr + 4 * (i + 256 * u));
    }
    float mm = -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u) mm = fmaxf(mm, fmaxf(fmaxf(a[u][0], a[u][1]), fmaxf(a[u][2], a[u][3])));
    if (mm > c.m) { const float f = __expf(c.m - mm); c.s *= f; c.t *= f; if (KL) c.u *= f; c.m = mm; }
    if (KL) {                              // the reference row's log-sum-exp: the policy row's operations, on its own state
      float mq = -INFINITY;
#pragma unroll
      for (int u = 0; u < 4; ++u) mq = fmaxf(mq, fmaxf(fmaxf(r[u][0], r[u][1]), fmaxf(r[u][2], r[u][3])));
      if (mq > c.mr) { const float f = __expf(c.mr - mq); c.sr *= f; c.mr = mq; }
    }
    float mu = c.m, mq = c.mr;
#pragma unroll
    for (int u = 0; u < 4; ++u) {          // (both rows' group u is consumed here: its eight registers are free afterwards)
      // With a reference row, a group's exponentials wait for the previous group's sums (an empty statement the compiler
      // cannot look through; the values are unchanged): scheduled freely, all 32 exponentials are hoisted above their use and
      // the kernel takes 76 VGPRs, 6 waves per SIMD instead of the 8 of the pair without a reference.
      if (KL) asm volatile("" : "+v"(mu), "+v"(mq) : "v"(c.s), "v"(c.t), "v"(c.u), "v"(c.sr));
      const float e0 = ex(a[u][0], mu), e1 = ex(a[u][1], mu), e2 = ex(a[u][2], mu), e3 = ex(a[u][3], mu);
      c.s += e0 + e1 + e2 + e3;
      c.t += ez(e0, a[u][0]) + ez(e1, a[u][1]) + ez(e2, a[u][2]) + ez(e3, a[u][3]);
      if (KL) {
        c.u += eu(e0, a[u][0], r[u][0]) + eu(e1, a[u][1], r[u][1]) + eu(e2, a[u][2], r[u][2]) + eu(e3, a[u][3], r[u][3]);
        const float q0 = ex(r[u][0], mq), q1 = ex(r[u][1], mq), q2 = ex(r[u][2], mq), q3 = ex(r[u][3], mq);
        c.sr += q0 + q1 + q2 + q3;
      }
    }
  }
  for (; i < nv; i += 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(z + 4 * i);
    const float mm = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
    if (mm > c.m) { const float f = __expf(c.m - mm); c.s *= f; c.t *= f; if (KL) c.u *= f; c.m = mm; }
    const float e0 = ex(a[0], c.m), e1 = ex(a[1], c.m), e2 = ex(a[2], c.m), e3 = ex(a[3], c.m);
    c.s += e0 + e1 + e2 + e3;
    c.t += ez(e0, a[0]) + ez(e1, a[1]) + ez(e2, a[2]) + ez(e3, a[3]);
    if (KL) {
      const f32x4 r = load4<RV>(zr + 4 * i);
      c.u += eu(e0, a[0], r[0]) + eu(e1, a[1], r[1]) + eu(e2, a[2], r[2]) + eu(e3, a[3], r[3]);
      const float mq = fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3]));
      if (mq > c.mr) { const float f = __expf(c.mr - mq); c.sr *= f; c.mr = mq; }
      const float q0 = ex(r[0], c.mr), q1 = ex(r[1], c.mr), q2 = ex(r[2], c.mr), q3 = ex(r[3], c.mr);
      c.sr += q0 + q1 + q2 + q3;
    }
  }
}

// log-sum-exp and entropy of one fp32 row in one read (16-byte loads when `vec`), block-wide.  m and s take the values of
// loss.hip's row_lse operation for operation (the likelihood step and the policy step with integer advantages agree bit for
// bit, tests/test_gpu_policy_model.py: keep the two in step); t rides along.  KL: the reference row zr is read beside it, column
// for column in the policy row's order (so its 16-byte loads need `rvec` AND `vec`: with a policy row on the scalar path both
// rows are read one column at a time), and kl = KL(softmax z || softmax zr), ref_lse = the reference row's log-sum-exp, which
// takes the policy row's operation sequence: zr == z gives ref_lse == lse bitwise and kl == +0.
template <bool KL>
__device__ __forceinline__ void row_lse_ent(const float* __restrict__ z, const float* __restrict__ zr, int V, bool vec, bool rvec,
                                            float* red, float& lse, float& ent, float& kl, float& ref_lse) {
  RowAcc c;
  if (vec) {
    const int nv = V >> 2;
    if (!KL || rvec) row_vector<KL, true>(z, zr, nv, c);
    else row_vector<KL, false>(z, zr, nv, c);
    row_scalar<KL>(z, zr, (nv << 2) + threadIdx.x, V, c);
  } else {
    row_scalar<KL>(z, zr, threadIdx.x, V, c);
  }
  const float gm = block_max(c.m, red);
  const float f = c.m == -INFINITY ? 0.f : __expf(c.m - gm);
  const float gs = block_sum(c.m == -INFINITY ? 0.f : c.s * f, red);
  const float gt = block_sum(c.m == -INFINITY ? 0.f : c.t * f, red);
  lse = gm + logf(gs);
  ent = lse - gt / gs;
  if (KL) {
    const float gu = block_sum(c.m == -INFINITY ? 0.f : c.u * f, red);
    const float gmr = block_max(c.mr, red);
    const float fr = c.mr == -INFINITY ? 0.f : __expf(c.mr - gmr);
    const float gsr = block_sum(c.mr == -INFINITY ? 0.f : c.sr * fr, red);
    ref_lse = gmr + logf(gsr);
    kl = gu / gs - lse + ref_lse;
  }
}

// the row's label, advantage and behaviour log-probability: adv / blogp are indexed by pos[row] (the row's flat position
// b * T + t) or by the row itself; a position outside [0, n_adv) makes the row an ignored one
__device__ __forceinline__ int row_inputs(int row, const int32_t* __restrict__ labels, const int32_t* __restrict__ pos,
                                          const float* __restrict__ adv, const float* __restrict__ blogp, int n_adv, int mode,
                                          float& A, float& b) {
  const int p = pos != nullptr ? pos[row] : row;
  A = 0.f;
  b = 0.f;
  if (p < 0 || p >= n_adv) return -1;
  A = adv[p];
  if (mode == PG_RATIO) b = blogp[p];
  return labels[row];
}

// KL = false: unimm_pg_loss_fwd (ref_logits .. ref_lse_o unused).  KL = true: the reference row is streamed beside the policy
// row, rowloss gains kl_coef * KL as its own addend (kl_coef == 0: nothing is added), kl and ref_lse are written.
template <bool KL>
__global__ __launch_bounds__(256) void pg_loss_fwd_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ pos, const float* __restrict__ adv,
                                                          const float* __restrict__ blogp, int n_adv, int mode, float eps,
                                                          float beta, float* __restrict__ rowloss, float* __restrict__ rownll,
                                                          float* __restrict__ lse_o, float* __restrict__ ent_o, int V, int ld,
                                                          const int32_t* __restrict__ n_dev,
                                                          const float* __restrict__ ref_logits, int ld_ref, float kl_coef,
                                                          float* __restrict__ kl_o, float* __restrict__ ref_lse_o) {
  __shared__ float red[4];
  const int row = blockIdx.x;
  if (n_dev != nullptr && row >= n_dev[0]) return;      // rows of the launch's capacity beyond the step's real count
  const float* z = logits + (size_t)row * ld;
  const float* zr = KL ? ref_logits + (size_t)row * ld_ref : nullptr;
  float lse, ent, kl = 0.f, ref_lse = 0.f;
  row_lse_ent<KL>(z, zr, V, (ld & 3) == 0, KL && (ld_ref & 3) == 0, red, lse, ent, kl, ref_lse);
  if (threadIdx.x == 0) {
    float A, b;
    const int y = row_inputs(row, labels, pos, adv, blogp, n_adv, mode, A, b);
    float loss = 0.f, nll = 0.f;
    if (y >= 0) {
      const float logp = z[y] - lse;
      nll = -logp;
      float surr = 0.f;                                  // a zero advantage contributes nothing, whatever log p_y is
      if (A != 0.f) {
        if (mode == PG_RATIO) {
          const float r = expf(logp - b);
          surr = fminf(r * A, fminf(fmaxf(r, 1.0f - eps), 1.0f + eps) * A);
        } else {
          surr = A * logp;
        }
      }
      loss = -surr;
      if (beta != 0.f) loss -= beta * ent;
      if (KL && kl_coef != 0.f) loss += kl_coef * kl;
    }
    rowloss[row] = loss;
    rownll[row] = nll;
    lse_o[row] = lse;
    ent_o[row] = ent;
    if (KL) {
      kl_o[row] = y >= 0 ? kl : 0.f;
      ref_lse_o[row] = ref_lse;
    }
  }
}

// KL = false: unimm_pg_loss_bwd.  KL = true: the gradient gains g inv kl_coef p_i ((z_i - lse) - (zr_i - ref_lse) - KL) as its own
// addend, skipped where it is zero (a row whose reference equals it keeps the bits of the gradient without the term) and where
// p_i = 0; each of the two rows takes 16-byte loads when its own stride allows.
template <bool KL>
__global__ __launch_bounds__(256) void pg_loss_bwd_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ pos, const float* __restrict__ adv,
                                                          const float* __restrict__ blogp, int n_adv, int mode, float eps,
                                                          float beta, const float* __restrict__ lse_i,
                                                          const float* __restrict__ ent_i, const float* __restrict__ g,
                                                          float inv_denom, bf16_t* __restrict__ dlogits, int V, int ld, int ldd,
                                                          const int32_t* __restrict__ n_dev, const float* __restrict__ inv_dev,
                                                          const float* __restrict__ ref_logits, int ld_ref, float kl_coef,
                                                          const float* __restrict__ kl_i, const float* __restrict__ ref_lse_i) {
  const int row = blockIdx.x;
  if (n_dev != nullptr && row >= n_dev[0]) return;
  if (inv_dev != nullptr) inv_denom = inv_dev[0];
  const float* z = logits + (size_t)row * ld;
  const float* zr = KL ? ref_logits + (size_t)row * ld_ref : nullptr;
  bf16_t* dz = dlogits + (size_t)row * ldd;
  float A, b;
  const int y = row_inputs(row, labels, pos, adv, blogp, n_adv, mode, A, b);
  const float lse = lse_i[row];
  float coef = 0.f, cent = 0.f, H = 0.f, ckl = 0.f, Dkl = 0.f, rlse = 0.f;
  if (y >= 0) {
    const float gs = g[0] * inv_denom;
    coef = gs * A;
    if (mode == PG_RATIO && A != 0.f) {
      const float r = expf((z[y] - lse) - b);
      // the clipped branch is the strict minimum: the surrogate is flat in the logits there
      const bool clipped = (A > 0.f && r > 1.0f + eps) || (A < 0.f && r < 1.0f - eps);
      coef = clipped ? 0.f : coef * r;
    }
    if (beta != 0.f) { cent = gs * beta; H = ent_i[row]; }
    if (KL && kl_coef != 0.f) { ckl = gs * kl_coef; Dkl = kl_i[row]; rlse = ref_lse_i[row]; }
  }
  const int n8 = ldd >> 3;
  if (coef == 0.f && cent == 0.f && ckl == 0.f) {        // ignored, clipped or zero-advantage rows: zeros, the logits are not read
    for (int i = threadIdx.x; i < n8; i += 256) *reinterpret_cast<u32x4*>(dz + 8 * i) = u32x4{0u, 0u, 0u, 0u};
    return;
  }
  // 8 columns per lane and iteration: two 16-byte loads, one 16-byte store (ldd % 8 == 0; columns >= V are written as
  // zeros: K padding of the dgrad GEMM).  Rows of the logits are 16-byte aligned when ld % 4 == 0.
  const bool vec = (ld & 3) == 0;
  const bool rvec = KL && (ld_ref & 3) == 0;
  const bool with_ent = cent != 0.f;
  const bool with_kl = KL && ckl != 0.f;
  // a row the pair without a reference fills with +0 (above) is here for its KL term alone: it starts from that +0, not from
  // coef * (p - [i == y]) = -0 on the label, so that a zero KL term leaves the other pair's bits
  const bool kl_only = KL && coef == 0.f && cent == 0.f;
  for (int i = threadIdx.x; i < n8; i += 256) {
    const int c0 = 8 * i;
    float v[8], q[8];
    const bool full = vec && c0 + 8 <= V;
    if (full) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(z + c0), b2 = *reinterpret_cast<const f32x4*>(z + c0 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b2[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (c0 + e < V) ? z[c0 + e] : -INFINITY;
    }
    if (with_kl) {                                       // the reference row's columns (never past V; unused where p_i = 0)
      if (rvec && c0 + 8 <= V) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(zr + c0), b2 = *reinterpret_cast<const f32x4*>(zr + c0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { q[e] = a[e]; q[4 + e] = b2[e]; }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = (c0 + e < V) ? zr[c0 + e] : 0.f;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + e;
      const float lp = v[e] - lse;
      const float p = __expf(lp);
      float d = kl_only ? 0.f : coef * (p - (c == y ? 1.0f : 0.0f));
      if (with_ent && p > 0.f) d += cent * (p * (lp + H));   // p_i = 0: the entropy term is 0, not 0 * -inf
      if (with_kl && p > 0.f) {                              // p_i = 0: the KL term is 0 whatever the reference holds
        const float k = ckl * (p * ((lp - (q[e] - rlse)) - Dkl));
        if (k != 0.f) d += k;                                // a zero term leaves d's bits (the sign of a zero included)
      }
      v[e] = (full || c < V) ? d : 0.f;
    }
    *reinterpret_cast<u32x4*>(dz + c0) = u32x4{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
  }
}

int pg_args_bad(const float* blogp, int mode, float clip_eps, float beta) {
  return (mode != PG_LOGP && mode != PG_RATIO) || (mode == PG_RATIO && !blogp) || !(clip_eps >= 0.f) || !(beta == beta);
}
// the reference row and the penalty's weight: a row at least V wide, kl_coef finite and >= 0
int kl_args_bad(const float* ref_logits, int ld_ref, int V, float kl_coef, const float* kl, const float* ref_lse) {
  return !ref_logits || !kl || !ref_lse || ld_ref < V || !(kl_coef >= 0.f) || !(kl_coef < INFINITY);
}

}  // namespace

extern "C" int unimm_pg_loss_fwd(const float* logits, const int32_t* labels, const int32_t* pos, const float* adv,
                                 const float* blogp, int32_t n_adv, int32_t mode, float clip_eps, float beta, float* rowloss,
                                 float* rownll, float* lse, float* ent, int32_t n, int32_t V, int32_t ld, const int32_t* n_dev,
                                 void* stream) {
  if (!logits || !labels || !adv || !rowloss || !rownll || !lse || !ent) return UNIMM_E_ARG;
  if (pg_args_bad(blogp, mode, clip_eps, beta)) return UNIMM_E_ARG;
  if (n <= 0 || V <= 0 || V > 65536 || ld < V || n_adv <= 0 || (pos == nullptr && n_adv < n)) return UNIMM_E_SHAPE;
  hipLaunchKernelGGL(pg_loss_fwd_kernel<false>, dim3(n), dim3(256), 0, (hipStream_t)stream, logits, labels, pos, adv, blogp, n_adv,
                     mode, clip_eps, beta, rowloss, rownll, lse, ent, V, ld, n_dev, nullptr, 0, 0.f, nullptr, nullptr);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

extern "C" int unimm_pg_loss_bwd(const float* logits, const int32_t* labels, const int32_t* pos, const float* adv,
                                 const float* blogp, int32_t n_adv, int32_t mode, float clip_eps, float beta, const float* lse,
                                 const float* ent, const float* g, float inv_denom, void* dlogits, int32_t n, int32_t V,
                                 int32_t ld, int32_t ldd, const int32_t* n_dev, const float* inv_dev, void* stream) {
  if (!logits || !labels || !adv || !lse || !ent || !g || !dlogits) return UNIMM_E_ARG;
  if (pg_args_bad(blogp, mode, clip_eps, beta)) return UNIMM_E_ARG;
  if (n <= 0 || V <= 0 || V > 65536 || ld < V || ldd < V || (ldd % 8) || n_adv <= 0 || (pos == nullptr && n_adv < n))
    return UNIMM_E_SHAPE;
  hipLaunchKernelGGL(pg_loss_bwd_kernel<false>, dim3(n), dim3(256), 0, (hipStream_t)stream, logits, labels, pos, adv, blogp, n_adv,
                     mode, clip_eps, beta, lse, ent, g, inv_denom, (bf16_t*)dlogits, V, ld, ldd, n_dev, inv_dev, nullptr, 0, 0.f,
                     nullptr, nullptr);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

extern "C" int unimm_pg_kl_loss_fwd(const float* logits, const int32_t* labels, const int32_t* pos, const float* adv,
                                    const float* blogp, int32_t n_adv, int32_t mode, float clip_eps, float beta, float* rowloss,
                                    float* rownll, float* lse, float* ent, int32_t n, int32_t V, int32_t ld, const int32_t* n_dev,
                                    const float* ref_logits, int32_t ld_ref, float kl_coef, float* kl, float* ref_lse,
                                    void* stream) {
  if (!logits || !labels || !adv || !rowloss || !rownll || !lse || !ent) return UNIMM_E_ARG;
  if (pg_args_bad(blogp, mode, clip_eps, beta) || kl_args_bad(ref_logits, ld_ref, V, kl_coef, kl, ref_lse)) return UNIMM_E_ARG;
  if (n <= 0 || V <= 0 || V > 65536 || ld < V || n_adv <= 0 || (pos == nullptr && n_adv < n)) return UNIMM_E_SHAPE;
  hipLaunchKernelGGL(pg_loss_fwd_kernel<true>, dim3(n), dim3(256), 0, (hipStream_t)stream, logits, labels, pos, adv, blogp, n_adv,
                     mode, clip_eps, beta, rowloss, rownll, lse, ent, V, ld, n_dev, ref_logits, ld_ref, kl_coef, kl, ref_lse);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

extern "C" int unimm_pg_kl_loss_bwd(const float* logits, const int32_t* labels, const int32_t* pos, const float* adv,
                                    const float* blogp, int32_t n_adv, int32_t mode, float clip_eps, float beta, const float* lse,
                                    const float* ent, const float* g, float inv_denom, void* dlogits, int32_t n, int32_t V,
                                    int32_t ld, int32_t ldd, const int32_t* n_dev, const float* inv_dev, const float* ref_logits,
                                    int32_t ld_ref, float kl_coef, const float* kl, const float* ref_lse, void* stream) {
  if (!logits || !labels || !adv || !lse || !ent || !g || !dlogits) return UNIMM_E_ARG;
  if (pg_args_bad(blogp, mode, clip_eps, beta) || kl_args_bad(ref_logits, ld_ref, V, kl_coef, kl, ref_lse)) return UNIMM_E_ARG;
  if (n <= 0 || V <= 0 || V > 65536 || ld < V || ldd < V || (ldd % 8) || n_adv <= 0 || (pos == nullptr && n_adv < n))
    return UNIMM_E_SHAPE;
  hipLaunchKernelGGL(pg_loss_bwd_kernel<true>, dim3(n), dim3(256), 0, (hipStream_t)stream, logits, labels, pos, adv, blogp, n_adv,
                     mode, clip_eps, beta, lse, ent, g, inv_denom, (bf16_t*)dlogits, V, ld, ldd, n_dev, inv_dev, ref_logits, ld_ref,
                     kl_coef, kl, ref_lse);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}
