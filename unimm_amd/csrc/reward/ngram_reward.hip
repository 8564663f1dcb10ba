// unimm_ngram_reward (include/unimm_reward.h; this directory is built into libunimm_reward.so, the extension library of
// libunimm_hip.so): the CIDEr-D consensus reward of S hypothesis rows against the references of their dialogs.  The definition,
// the table and the limits are stated in the header; tests/reward_ref.py restates the definition in float64 Python.
//
// One 256-thread workgroup per hypothesis row.  Wave w holds order n = w + 1, lane p the window at position p, once for the
// hypothesis (its key, tf, first-occurrence flag and v_h = tf * idf stay in registers for the whole walk) and once more for
// each reference in turn.  Per reference j, in index order, with three workgroup barriers:
//   1  the reference's L_r tokens go to LDS;
//   2  lane p < L_r - n + 1 counts its window's tf over the reference, looks its idf up and writes v_r and (at the window's first
//      position) v_r^2 to LDS;
//   3  hypothesis lane p (first positions only) finds its window in the reference and writes min(v_h, v_r) * v_r to LDS;
//   4  lane 0 of each wave adds the order's terms and the reference's squares, each a serial chain in position order (the entries
//      of repeated windows are +0.0 and change no bit), divides, applies the length factor and adds w_j * val to the row's c_n.
// No atomics, no arrival counters, fp64 throughout: equal inputs give equal bits, and a row reads nothing but its own inputs.
// Tokens at or past an answer's effective length are never loaded.
#include <math.h>

#include "../../../include/unimm_reward.h"
#include "../common.h"

namespace {

constexpr int NTHREADS = 256;
constexpr int LMAX = UNIMM_REWARD_MAX_LEN;
constexpr int ORDERS = UNIMM_REWARD_ORDERS;
static_assert(NTHREADS == ORDERS * LMAX && LMAX == 64, "one wave per order, one lane per position");

struct RewardParams {
  const int32_t *hyp, *hyp_len, *hyp_group, *ref, *ref_len;
  const float* ref_weight;
  const int32_t* keys;
  const double* idf;
  float* reward;
  double* per_order;
  double default_idf, two_sigma2;
  int ldh, G, M, ldr, cap, max_hyp_len, max_ref_len;
};

__device__ __forceinline__ double lookup_idf(const RewardParams& a, const int (&k)[4]) {
  if (a.keys == nullptr) return 1.0;
  uint32_t h = (uint32_t)UNIMM_NGRAM_HASH_BASIS;
#pragma unroll
  for (int i = 0; i < 4; ++i) h = (h ^ (uint32_t)k[i]) * (uint32_t)UNIMM_NGRAM_HASH_PRIME;
  h ^= h >> 16;
  const uint32_t mask = (uint32_t)a.cap - 1u;
  uint32_t slot = h & mask;
  for (int probe = 0; probe < a.cap; ++probe) {
    const int32_t* e = a.keys + (size_t)slot * 4;
    const int e0 = e[0];
    if (e0 == UNIMM_NGRAM_EMPTY) break;
    if (e0 == k[0] && e[1] == k[1] && e[2] == k[2] && e[3] == k[3]) return a.idf[slot];
    slot = (slot + 1u) & mask;
  }
  return a.default_idf;
}

// the window of n tokens at position p of tok[0:L] (p + n <= L): its key, its count over the answer, whether p is its first position
__device__ __forceinline__ void window(const int* tok, int L, int n, int p, int (&k)[4], int& tf, bool& first) {
#pragma unroll
  for (int e = 0; e < 4; ++e) k[e] = e < n ? tok[p + e] : -1;
  tf = 0;
  first = true;
  for (int q = 0; q + n <= L; ++q) {
    bool eq = true;
#pragma unroll
    for (int e = 0; e < 4; ++e) eq = eq && (e >= n || tok[q + e] == k[e]);
    tf += eq ? 1 : 0;
    first = first && !(eq && q < p);
  }
}

__global__ __launch_bounds__(NTHREADS) void ngram_reward_kernel(RewardParams a) {
  __shared__ int ht[LMAX + 4], rt[LMAX + 4];     // + 4: `window` may form the address of tok[q + e], e >= n, which it never reads
  __shared__ double rv[ORDERS][LMAX], rsq[ORDERS][LMAX], term[ORDERS][LMAX];
  __shared__ double cn[ORDERS];
  const int tid = threadIdx.x, s = blockIdx.x, w = tid >> 6, p = tid & 63, n = w + 1;
  const int Lh = min(a.hyp_len[s], a.max_hyp_len) - 1;
  const int g = a.hyp_group[s];
  if (Lh <= 0 || g < 0 || g >= a.G) {            // uniform over the workgroup
    if (tid == 0) a.reward[s] = 0.f;
    if (tid < ORDERS && a.per_order != nullptr) a.per_order[(size_t)s * ORDERS + tid] = 0.0;
    return;
  }
  if (tid < Lh) ht[tid] = a.hyp[(size_t)s * a.ldh + tid];
  __syncthreads();
  const int nh = Lh - n + 1;                     // the hypothesis' windows of this order (<= 0: none)
  int hk[4] = {-1, -1, -1, -1};
  double vh = 0.0;
  bool hfirst = false;
  if (p < nh) {
    int tf;
    window(ht, Lh, n, p, hk, tf, hfirst);
    vh = (double)tf * lookup_idf(a, hk);
  }
  term[w][p] = hfirst ? vh * vh : 0.0;
  __syncthreads();
  double normh = 0.0;
  if (p == 0) {
    double s2 = 0.0;
    for (int q = 0; q < nh; ++q) s2 = s2 + term[w][q];
    normh = sqrt(s2);
  }
  __syncthreads();

  double acc = 0.0, wsum = 0.0;                  // lane 0 of each wave: sum_j w_j val_n(h, r_j), sum_j w_j
  const size_t gm = (size_t)g * a.M;
  for (int j = 0; j < a.M; ++j) {                // every branch on j's length or weight is uniform over the workgroup
    const int rl = a.ref_len[gm + j];
    if (rl <= 0) continue;                       // absent
    const double wj = a.ref_weight != nullptr ? (double)a.ref_weight[gm + j] : 1.0;
    if (wj == 0.0) continue;                     // adds exactly 0 to both sums
    const int Lr = min(rl, a.max_ref_len) - 1;
    if (Lr <= 0) {                               // present and empty: 0, and it counts in the denominator
      wsum = wsum + wj;
      continue;
    }
    if (tid < Lr) rt[tid] = a.ref[(gm + j) * (size_t)a.ldr + tid];
    __syncthreads();
    const int nr = Lr - n + 1;
    if (p < nr) {
      int rk[4], tf;
      bool first;
      window(rt, Lr, n, p, rk, tf, first);
      const double v = (double)tf * lookup_idf(a, rk);
      rv[w][p] = v;
      rsq[w][p] = first ? v * v : 0.0;
    }
    __syncthreads();
    double t = 0.0;
    if (hfirst) {
      for (int q = 0; q < nr; ++q) {
        bool eq = true;
#pragma unroll
        for (int e = 0; e < 4; ++e) eq = eq && (e >= n || rt[q + e] == hk[e]);
        if (eq) {
          const double vr = rv[w][q];
          t = fmin(vh, vr) * vr;
          break;
        }
      }
    }
    term[w][p] = t;
    __syncthreads();
    if (p == 0) {
      double num = 0.0, r2 = 0.0;
      for (int q = 0; q < nh; ++q) num = num + term[w][q];
      for (int q = 0; q < nr; ++q) r2 = r2 + rsq[w][q];
      const double den = normh * sqrt(r2);
      double val = num;
      if (den != 0.0) val = num / den;
      const double d = (double)(Lh - Lr);
      val = val * exp(-(d * d) / a.two_sigma2);
      acc = acc + wj * val;
      wsum = wsum + wj;
    }
  }
  if (p == 0) cn[w] = wsum != 0.0 ? acc / wsum : 0.0;
  __syncthreads();
  if (tid == 0) a.reward[s] = (float)(10.0 * (((cn[0] + cn[1]) + cn[2]) + cn[3]) / 4.0);
  if (tid < ORDERS && a.per_order != nullptr) a.per_order[(size_t)s * ORDERS + tid] = cn[tid];
}

}  // namespace

extern "C" int unimm_reward_version(void) { return 1; }

extern "C" int unimm_ngram_reward(const unimm_ngram_reward_args* a, void* stream) {
  if (a == nullptr) return UNIMM_E_ARG;
  if (a->S < 0) return UNIMM_E_SHAPE;
  if (a->S == 0) return UNIMM_OK;                // no rows: nothing to check (an empty tensor's address is NULL), nothing to launch
  if (a->hyp == nullptr || a->hyp_len == nullptr || a->hyp_group == nullptr || a->ref == nullptr || a->ref_len == nullptr ||
      a->reward == nullptr)
    return UNIMM_E_ARG;
  if ((a->table_keys == nullptr) != (a->table_idf == nullptr)) return UNIMM_E_ARG;
  if (!(a->sigma > 0.0)) return UNIMM_E_ARG;     // NaN too
  if (a->G < 1 || a->M < 1 || a->M > UNIMM_REWARD_MAX_REFS || a->ldh < 1 || a->ldr < 1) return UNIMM_E_SHAPE;
  if (a->max_hyp_len < 0 || a->max_hyp_len > LMAX + 1 || a->max_hyp_len > a->ldh) return UNIMM_E_SHAPE;
  if (a->max_ref_len < 0 || a->max_ref_len > LMAX + 1 || a->max_ref_len > a->ldr) return UNIMM_E_SHAPE;
  if (a->table_keys != nullptr && (a->cap < 1 || (a->cap & (a->cap - 1)) != 0)) return UNIMM_E_SHAPE;
  RewardParams p;
  p.hyp = a->hyp; p.hyp_len = a->hyp_len; p.hyp_group = a->hyp_group; p.ref = a->ref; p.ref_len = a->ref_len;
  p.ref_weight = a->ref_weight; p.keys = a->table_keys; p.idf = a->table_idf; p.reward = a->reward; p.per_order = a->per_order;
  p.default_idf = a->default_idf; p.two_sigma2 = 2.0 * a->sigma * a->sigma;
  p.ldh = a->ldh; p.G = a->G; p.M = a->M; p.ldr = a->ldr; p.cap = a->cap;
  p.max_hyp_len = a->max_hyp_len; p.max_ref_len = a->max_ref_len;
  hipLaunchKernelGGL(ngram_reward_kernel, dim3((unsigned)a->S), dim3(NTHREADS), 0, (hipStream_t)stream, p);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}
