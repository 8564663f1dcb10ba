// Policy-gradient objective on the decoded rows of sampled answers (gfx950): REINFORCE / self-critical (A log p_y), the
// clipped importance-weighted surrogate (min(r A, clamp(r, 1-eps, 1+eps) A), r = p_y / q_y) and an entropy bonus -- forward and
// backward.  The layout is that of the likelihood kernels (csrc/loss.hip): one 256-lane workgroup per row, fp32 logits read
// once per direction, device-side row count and denominator.  The row's entropy comes out of the SAME pass as its
// log-sum-exp: next to the running maximum m and s = sum e^(z-m) a lane keeps t = sum e^(z-m) z, rescaled with s, and
// H = -sum p log p = lse - t / s.
// The KL-regularised pair (unimm_pg_kl_loss_*) streams a frozen reference's row beside the policy's in the same pass: a lane
// also keeps u = sum e^(z-m) (z - zr) and the reference row's own (mr, sr), and KL(p || pr) = u / s - lse + ref_lse.  Both
// pairs are instantiations of one template, so the policy row's m, s, t are computed by the same source either way.
// The listwise preference objective over whole candidate answers (unimm_seq_pref, at the end of this file) reads no logits: it
// turns the likelihood kernel's per-row -log p_y into one coefficient per row for the backward kernel above.
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

// ---------------------------------------------------------------------------------------------------------------------------
// Listwise preference over the likelihoods of whole candidate answers (unimm_seq_pref, include/unimm_hip.h): per-row -log p_y
// -> per-sequence scores -> a softmax over each group's sequences against the target weights -> one coefficient per row, which
// unimm_pg_loss_bwd (LOGP mode) turns into the logits' gradient.  A few thousand floats: everything is fp64 and every sum a
// serial chain in index order, so the result does not depend on the launch.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

// the workspace: fp64 D [B] | fp32 c [B] | int32 L [B] | int32 alive [groups]
struct PrefWs {
  double* D;
  float* c;
  int32_t* L;
  int32_t* alive;
};
__device__ __forceinline__ PrefWs pref_ws(void* ws, int B) {
  char* p = static_cast<char*>(ws);
  return PrefWs{reinterpret_cast<double*>(p), reinterpret_cast<float*>(p + 8 * (size_t)B),
                reinterpret_cast<int32_t*>(p + 12 * (size_t)B), reinterpret_cast<int32_t*>(p + 16 * (size_t)B)};
}
// the rows of this launch: n is a capacity when the device word is given
__device__ __forceinline__ int pref_rows(int n, const int32_t* __restrict__ n_dev) {
  const int m = n_dev != nullptr ? min(n, n_dev[0]) : n;
  return m > 0 ? m : 0;
}

// One wave per sequence j.  The wave walks the rows 64 at a time; the lanes whose row belongs to j vote, and the rows voted
// for are added one after the other in ascending index (every lane does the same additions: the loads are wave-uniform).
__global__ __launch_bounds__(256) void pref_seq_kernel(const float* __restrict__ rownll, const float* __restrict__ ref_rownll,
                                                       const int32_t* __restrict__ row_seq, int n,
                                                       const int32_t* __restrict__ n_dev, int B, int lnorm,
                                                       float* __restrict__ seq_score, float* __restrict__ seq_prob, void* wsp) {
  const int rows = pref_rows(n, n_dev);
  if (rows == 0) return;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= B) return;
  const int lane = threadIdx.x & 63;
  double S = 0.0, R = 0.0;
  int cnt = 0;
  for (int base = 0; base < rows; base += 64) {
    const int r = base + lane;
    unsigned long long votes = __ballot(r < rows && row_seq[r] == j);
    while (votes != 0ull) {
      const int rr = base + __ffsll(votes) - 1;
      votes &= votes - 1ull;
      S -= (double)rownll[rr];
      if (ref_rownll != nullptr) R -= (double)ref_rownll[rr];
      ++cnt;
    }
  }
  if (lane == 0) {
    const PrefWs ws = pref_ws(wsp, B);
    const double D = cnt > 0 ? (S - R) / (lnorm ? (double)cnt : 1.0) : (double)NAN;
    ws.D[j] = D;
    ws.L[j] = cnt;
    ws.c[j] = 0.f;                       // until its group says otherwise (pref_group_kernel)
    seq_score[j] = (float)D;
    seq_prob[j] = 0.f;
  }
}

// One workgroup per group g.  Its members -- the sequences of g that have rows -- are collected in ascending sequence index
// (a vote per wave, the waves' counts in LDS), at most UNIMM_PREF_MAX_MEMBERS of them; z, w and the terms of the sums live in
// LDS and lane 0 adds them in member order.
__global__ __launch_bounds__(256) void pref_group_kernel(const int32_t* __restrict__ seq_group, const float* __restrict__ seq_weight,
                                                         int n, const int32_t* __restrict__ n_dev, int B, float beta_f, int lnorm,
                                                         float* __restrict__ seq_prob, float* __restrict__ group_loss, void* wsp) {
  constexpr int MAXM = UNIMM_PREF_MAX_MEMBERS;
  __shared__ int mem[MAXM];
  __shared__ double zs[MAXM], wd[MAXM], tm[MAXM];
  __shared__ double bc[2];                // broadcast: log-sum-exp, W
  __shared__ int wcnt[4];
  __shared__ int bad;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (pref_rows(n, n_dev) == 0) {
    if (tid == 0) group_loss[g] = 0.f;
    return;
  }
  const PrefWs ws = pref_ws(wsp, B);
  if (tid == 0) bad = 0;
  int count = 0;                          // members so far (the same in every lane)
  for (int base = 0; base < B; base += 256) {
    const int j = base + tid;
    const bool hit = j < B && seq_group[j] == g && ws.L[j] > 0;
    const unsigned long long votes = __ballot(hit);
    if (lane == 0) wcnt[wave] = __popcll(votes);
    __syncthreads();
    int slot = count + __popcll(votes & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) slot += wcnt[w];
    if (hit && slot < MAXM) mem[slot] = j;
    count += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  const int M = count;
  if (M == 0) {                           // nobody to compare: not alive, loss 0
    if (tid == 0) { group_loss[g] = 0.f; ws.alive[g] = 0; }
    return;
  }
  double w = 0.0, Lp = 1.0;
  int j = -1;
  if (M <= MAXM && tid < M) {
    j = mem[tid];
    const float wf = seq_weight[j];
    if (!(wf >= 0.f && wf < INFINITY)) bad = 1;
    w = (double)wf;
    Lp = lnorm ? (double)ws.L[j] : 1.0;
    zs[tid] = (double)beta_f * ws.D[j];
    wd[tid] = w;
  }
  __syncthreads();
  if (M > MAXM || bad != 0) {             // more members than a slate holds, or a weight that is no weight: NaN, not alive
    for (int k = tid; k < B; k += 256)
      if (seq_group[k] == g && ws.L[k] > 0) seq_prob[k] = NAN;
    if (tid == 0) { group_loss[g] = NAN; ws.alive[g] = 0; }
    return;
  }
  double m = -INFINITY;
  for (int k = 0; k < M; ++k) m = fmax(m, zs[k]);
  if (tid < M) tm[tid] = exp(zs[tid] - m);
  __syncthreads();
  if (tid == 0) {
    double s = 0.0, W = 0.0;
    for (int k = 0; k < M; ++k) s += tm[k];
    for (int k = 0; k < M; ++k) W += wd[k];
    bc[0] = m + log(s);
    bc[1] = W;
  }
  __syncthreads();
  const double lse = bc[0], W = bc[1];
  const bool alive = W > 0.0;
  if (tid < M) {
    const double logP = zs[tid] - lse;
    const double P = exp(logP);
    tm[tid] = w * logP;
    seq_prob[j] = (float)P;
    ws.c[j] = alive ? (float)((double)beta_f * (w - W * P) / Lp) : 0.f;
  }
  __syncthreads();
  if (tid == 0) {
    double loss = 0.0;
    for (int k = 0; k < M; ++k) loss += tm[k];
    group_loss[g] = alive ? (float)(-loss) : 0.f;
    ws.alive[g] = alive ? 1 : 0;
  }
}

// One lane per row: its sequence's coefficient.  Workgroup 0 also counts the groups that are alive (integers: any order).
__global__ __launch_bounds__(256) void pref_rows_kernel(const int32_t* __restrict__ row_seq, int n, const int32_t* __restrict__ n_dev,
                                                        int B, int groups, float* __restrict__ adv, float* __restrict__ alive_inv,
                                                        void* wsp) {
  __shared__ int red[4];
  const int rows = pref_rows(n, n_dev);
  const PrefWs ws = pref_ws(wsp, B);
  if (blockIdx.x == 0) {
    if (rows == 0) {
      if (threadIdx.x == 0) alive_inv[0] = NAN;
    } else {
      int cnt = 0;
      for (int g = threadIdx.x; g < groups; g += 256) cnt += ws.alive[g];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
      __syncthreads();
      if (threadIdx.x == 0) {
        const int alive = red[0] + red[1] + red[2] + red[3];
        alive_inv[0] = alive > 0 ? (float)(1.0 / (double)alive) : NAN;
      }
    }
  }
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < rows) {
    const int s = row_seq[r];
    adv[r] = (s >= 0 && s < B) ? ws.c[s] : 0.f;
  }
}

}  // namespace

extern "C" int unimm_seq_pref(const unimm_seq_pref_args* a, void* stream) {
  if (!a || !a->seq_group || !a->seq_weight || !a->seq_score || !a->seq_prob || !a->group_loss || !a->alive_inv || !a->workspace)
    return UNIMM_E_ARG;
  if (a->n > 0 && (!a->rownll || !a->row_seq || !a->adv)) return UNIMM_E_ARG;      // (arrays of n elements: not looked at when n == 0)
  if (!(a->beta > 0.f) || !(a->beta < INFINITY) || a->groups < 1 || a->B < 1 || a->n < 0) return UNIMM_E_ARG;
  if (a->workspace_bytes < (int64_t)UNIMM_PREF_WS_ITEM_BYTES * ((int64_t)a->B + (int64_t)a->groups)) return UNIMM_E_ARG;
  if (reinterpret_cast<uintptr_t>(a->workspace) & 15u) return UNIMM_E_ALIGN;
  const hipStream_t st = (hipStream_t)stream;
  const int lnorm = a->length_normalize != 0;
  if (a->n > 0) {
    hipLaunchKernelGGL(pref_seq_kernel, dim3((a->B + 3) / 4), dim3(256), 0, st, a->rownll, a->ref_rownll, a->row_seq, a->n, a->n_dev,
                       a->B, lnorm, a->seq_score, a->seq_prob, a->workspace);
    UNIMM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(pref_group_kernel, dim3(a->groups), dim3(256), 0, st, a->seq_group, a->seq_weight, a->n, a->n_dev, a->B, a->beta,
                     lnorm, a->seq_prob, a->group_loss, a->workspace);
  UNIMM_CHECK_LAUNCH();
  hipLaunchKernelGGL(pref_rows_kernel, dim3(a->n > 0 ? (a->n + 255) / 256 : 1), dim3(256), 0, st, a->row_seq, a->n, a->n_dev, a->B,
                     a->groups, a->adv, a->alive_inv, a->workspace);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}
