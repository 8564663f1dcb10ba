// Policy-gradient objective on the decoded rows of sampled answers (gfx950): REINFORCE / self-critical (A log p_y), the
// clipped importance-weighted surrogate (min(r A, clamp(r, 1-eps, 1+eps) A), r = p_y / q_y) and an entropy bonus -- forward and
// backward.  The layout is that of the likelihood kernels (csrc/loss.hip): one 256-lane workgroup per row, fp32 logits read
// once per direction, device-side row count and denominator.  The row's entropy comes out of the SAME pass as its
// log-sum-exp: next to the running maximum m and s = sum e^(z-m) a lane keeps t = sum e^(z-m) z, rescaled with s, and
// H = -sum p log p = lse - t / s.
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

// log-sum-exp and entropy of one fp32 row in one read (16-byte loads when `vec`), block-wide.  m and s take the values of
// loss.hip's row_lse operation for operation (the likelihood step and the policy step with integer advantages agree bit for
// bit, tests/test_gpu_policy_model.py: keep the two in step); t rides along.
__device__ __forceinline__ void row_lse_ent(const float* __restrict__ z, int V, bool vec, float* red, float& lse, float& ent) {
  float m = -INFINITY, s = 0.f, t = 0.f;
  if (vec) {
    const int nv = V >> 2;
    int i = threadIdx.x;
    for (; i + 768 < nv; i += 1024) {        // four 16-byte loads in flight per lane (the row is read once, from HBM)
      f32x4 a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = *reinterpret_cast<const f32x4*>(z + 4 * (i + 256 * u));
      float mm = -INFINITY;
#pragma unroll
      for (int u = 0; u < 4; ++u) mm = fmaxf(mm, fmaxf(fmaxf(a[u][0], a[u][1]), fmaxf(a[u][2], a[u][3])));
      if (mm > m) { const float f = __expf(m - mm); s *= f; t *= f; m = mm; }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float e0 = ex(a[u][0], m), e1 = ex(a[u][1], m), e2 = ex(a[u][2], m), e3 = ex(a[u][3], m);
        s += e0 + e1 + e2 + e3;
        t += ez(e0, a[u][0]) + ez(e1, a[u][1]) + ez(e2, a[u][2]) + ez(e3, a[u][3]);
      }
    }
    for (; i < nv; i += 256) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(z + 4 * i);
      const float mm = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
      if (mm > m) { const float f = __expf(m - mm); s *= f; t *= f; m = mm; }
      const float e0 = ex(a[0], m), e1 = ex(a[1], m), e2 = ex(a[2], m), e3 = ex(a[3], m);
      s += e0 + e1 + e2 + e3;
      t += ez(e0, a[0]) + ez(e1, a[1]) + ez(e2, a[2]) + ez(e3, a[3]);
    }
    for (int i = (nv << 2) + threadIdx.x; i < V; i += 256) {
      const float a = z[i];
      if (a > m) { const float f = __expf(m - a); s *= f; t *= f; m = a; }
      const float e = ex(a, m);
      s += e;
      t += ez(e, a);
    }
  } else {
    for (int i = threadIdx.x; i < V; i += 256) {
      const float a = z[i];
      if (a > m) { const float f = __expf(m - a); s *= f; t *= f; m = a; }
      const float e = ex(a, m);
      s += e;
      t += ez(e, a);
    }
  }
  const float gm = block_max(m, red);
  const float f = m == -INFINITY ? 0.f : __expf(m - gm);
  const float gs = block_sum(m == -INFINITY ? 0.f : s * f, red);
  const float gt = block_sum(m == -INFINITY ? 0.f : t * f, red);
  lse = gm + logf(gs);
  ent = lse - gt / gs;
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

__global__ __launch_bounds__(256) void pg_loss_fwd_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ pos, const float* __restrict__ adv,
                                                          const float* __restrict__ blogp, int n_adv, int mode, float eps,
                                                          float beta, float* __restrict__ rowloss, float* __restrict__ rownll,
                                                          float* __restrict__ lse_o, float* __restrict__ ent_o, int V, int ld,
                                                          const int32_t* __restrict__ n_dev) {
  __shared__ float red[4];
  const int row = blockIdx.x;
  if (n_dev != nullptr && row >= n_dev[0]) return;      // rows of the launch's capacity beyond the step's real count
  const float* z = logits + (size_t)row * ld;
  float lse, ent;
  row_lse_ent(z, V, (ld & 3) == 0, red, lse, ent);
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
    }
    rowloss[row] = loss;
    rownll[row] = nll;
    lse_o[row] = lse;
    ent_o[row] = ent;
  }
}

__global__ __launch_bounds__(256) void pg_loss_bwd_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ pos, const float* __restrict__ adv,
                                                          const float* __restrict__ blogp, int n_adv, int mode, float eps,
                                                          float beta, const float* __restrict__ lse_i,
                                                          const float* __restrict__ ent_i, const float* __restrict__ g,
                                                          float inv_denom, bf16_t* __restrict__ dlogits, int V, int ld, int ldd,
                                                          const int32_t* __restrict__ n_dev, const float* __restrict__ inv_dev) {
  const int row = blockIdx.x;
  if (n_dev != nullptr && row >= n_dev[0]) return;
  if (inv_dev != nullptr) inv_denom = inv_dev[0];
  const float* z = logits + (size_t)row * ld;
  bf16_t* dz = dlogits + (size_t)row * ldd;
  float A, b;
  const int y = row_inputs(row, labels, pos, adv, blogp, n_adv, mode, A, b);
  const float lse = lse_i[row];
  float coef = 0.f, cent = 0.f, H = 0.f;
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
  }
  const int n8 = ldd >> 3;
  if (coef == 0.f && cent == 0.f) {                      // ignored, clipped or zero-advantage rows: zeros, the logits are not read
    for (int i = threadIdx.x; i < n8; i += 256) *reinterpret_cast<u32x4*>(dz + 8 * i) = u32x4{0u, 0u, 0u, 0u};
    return;
  }
  // 8 columns per lane and iteration: two 16-byte loads, one 16-byte store (ldd % 8 == 0; columns >= V are written as
  // zeros: K padding of the dgrad GEMM).  Rows of the logits are 16-byte aligned when ld % 4 == 0.
  const bool vec = (ld & 3) == 0;
  const bool with_ent = cent != 0.f;
  for (int i = threadIdx.x; i < n8; i += 256) {
    const int c0 = 8 * i;
    float v[8];
    const bool full = vec && c0 + 8 <= V;
    if (full) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(z + c0), b2 = *reinterpret_cast<const f32x4*>(z + c0 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b2[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (c0 + e < V) ? z[c0 + e] : -INFINITY;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + e;
      const float lp = v[e] - lse;
      const float p = __expf(lp);
      float d = coef * (p - (c == y ? 1.0f : 0.0f));
      if (with_ent && p > 0.f) d += cent * (p * (lp + H));   // p_i = 0: the entropy term is 0, not 0 * -inf
      v[e] = (full || c < V) ? d : 0.f;
    }
    *reinterpret_cast<u32x4*>(dz + c0) = u32x4{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
  }
}

}  // namespace

extern "C" int unimm_pg_loss_fwd(const float* logits, const int32_t* labels, const int32_t* pos, const float* adv,
                                 const float* blogp, int32_t n_adv, int32_t mode, float clip_eps, float beta, float* rowloss,
                                 float* rownll, float* lse, float* ent, int32_t n, int32_t V, int32_t ld, const int32_t* n_dev,
                                 void* stream) {
  if (!logits || !labels || !adv || !rowloss || !rownll || !lse || !ent) return UNIMM_E_ARG;
  if ((mode != PG_LOGP && mode != PG_RATIO) || (mode == PG_RATIO && !blogp) || !(clip_eps >= 0.f) || !(beta == beta))
    return UNIMM_E_ARG;
  if (n <= 0 || V <= 0 || V > 65536 || ld < V || n_adv <= 0 || (pos == nullptr && n_adv < n)) return UNIMM_E_SHAPE;
  hipLaunchKernelGGL(pg_loss_fwd_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, logits, labels, pos, adv, blogp, n_adv,
                     mode, clip_eps, beta, rowloss, rownll, lse, ent, V, ld, n_dev);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

extern "C" int unimm_pg_loss_bwd(const float* logits, const int32_t* labels, const int32_t* pos, const float* adv,
                                 const float* blogp, int32_t n_adv, int32_t mode, float clip_eps, float beta, const float* lse,
                                 const float* ent, const float* g, float inv_denom, void* dlogits, int32_t n, int32_t V,
                                 int32_t ld, int32_t ldd, const int32_t* n_dev, const float* inv_dev, void* stream) {
  if (!logits || !labels || !adv || !lse || !ent || !g || !dlogits) return UNIMM_E_ARG;
  if ((mode != PG_LOGP && mode != PG_RATIO) || (mode == PG_RATIO && !blogp) || !(clip_eps >= 0.f) || !(beta == beta))
    return UNIMM_E_ARG;
  if (n <= 0 || V <= 0 || V > 65536 || ld < V || ldd < V || (ldd % 8) || n_adv <= 0 || (pos == nullptr && n_adv < n))
    return UNIMM_E_SHAPE;
  hipLaunchKernelGGL(pg_loss_bwd_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, logits, labels, pos, adv, blogp, n_adv,
                     mode, clip_eps, beta, lse, ent, g, inv_denom, (bf16_t*)dlogits, V, ld, ldd, n_dev, inv_dev);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}
