// unimm_lm_mix (include/unimm_mix.h; this directory is built into libunimm_mix.so, the extension library of libunimm_hip.so):
// K <= 5 fp32 logits rows of the same position -> ONE row, the members' next-token
// distributions mixed per id, for ensemble and contrastive answer generation (unimm_amd/generation.py).  One workgroup per row,
// as the other LM row kernels (generate.hip); the selection kernels run on the mixed row unchanged.
//
// Operation order (tests/mix_ref.py restates it in numpy float32).
//   LOGIT   z_i = w_0 * x_0,i, then z_i = z_i + w_m * x_m,i for m = 1 .. K-1 in order; every product is rounded to fp32 on its
//           own (`rounded` below keeps -ffp-contract=fast from fusing it into the sum), so the restatement is equal bit for bit.
//   PROB    per member m with w_m != 0, lse_m = logsumexp(x_m[0:V]): thread t folds the columns it visits, in ascending order,
//           into a pair (mx, s): mn = max(mx, chunk max); where mn > -inf, s = s * expf(mx - mn) + sum_e expf(x_e - mn) (e in
//           column order), mx = mn.  The scalar path visits one column at a time, j = t, t + 256, ...; the 16-byte path chunks of
//           four, j = 4 t, 4 t + 1024, ..., then the V % 4 tail columns one at a time.  Pairs combine over the wave by the xor
//           butterfly (o = 32 .. 1: M = max(mx, mx'), s = M == -inf ? 0 : s * expf(mx - M) + s' * expf(mx' - M)), the four waves in
//           order (M = max_w mx_w, tot = sum over the waves with mx_w > -inf of s_w * expf(mx_w - M)), lse_m = M + logf(tot).
//           Then per id: t_m = x_m,i > -inf ? (x_m,i - lse_m) + logf(w_m) : -inf; T = max_m t_m; z_i = -inf when T = -inf, else
//           T + logf(sum_m expf(t_m - T)), m ascending over the members with w_m != 0.  (Here the compiler may fuse a product
//           into the sum that follows it: one rounding fewer than the restatement, inside the budget tests/mix_ref.py states.)
//   CUT     (log_alpha > -inf) m0 = the largest x_0,i over the eligible ids, b = the smallest id that reaches it; thr = m0 +
//           log_alpha (one fp32 add); out_i = -inf where i != sep, i != b and x_0,i < thr; z_i elsewhere.
// Traffic: LOGIT without a cut reads every row once; with a cut member 0 twice; PROB every member with w_m != 0 twice.
#include <math.h>

#include <type_traits>

#include "../../../include/unimm_mix.h"
#include "../common.h"

namespace {

constexpr int NTHREADS = 256;
constexpr int NWAVES = NTHREADS / 64;
constexpr int KMAX = UNIMM_MIX_MAX_MEMBERS;
constexpr int VMAX = 65536;     // vocabulary bound of the banned-id bitmask

struct MixParams {
  const float* x[KMAX];
  float* out;
  const int32_t *banned, *flags;
  int ld[KMAX];
  float w[KMAX];
  int K, prob, cut, vec, rows, V, ldo, nbanned, sep;
  float log_alpha;
};

template <int W>
__device__ __forceinline__ void load_w(const float* p, float (&v)[W]) {
  if constexpr (W == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = p[0];
  }
}

template <int W>
__device__ __forceinline__ void store_w(float* p, const float (&v)[W]) {
  if constexpr (W == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0];
  }
}

// a value as it is rounded to fp32 HERE: the empty asm keeps a product from being fused into a later sum
__device__ __forceinline__ float rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

template <int W>
using width = std::integral_constant<int, W>;

__global__ __launch_bounds__(NTHREADS) void lm_mix_kernel(MixParams a) {
  __shared__ uint32_t ban[VMAX / 32];            // CUT only
  __shared__ float rm[KMAX][NWAVES], rs[KMAX][NWAVES];
  __shared__ float cv[NWAVES];
  __shared__ int ci[NWAVES];
  const int tid = threadIdx.x, row = blockIdx.x, wave = tid >> 6, lane = tid & 63;
  const int V = a.V, sep = a.sep;
  const bool prob = a.prob != 0, cut = a.cut != 0;
  const float* x[KMAX];
  bool used[KMAX];                               // the member's row enters z
#pragma unroll
  for (int m = 0; m < KMAX; ++m) {
    const bool in = m < a.K;
    x[m] = a.x[in ? m : 0] + (int64_t)row * a.ld[in ? m : 0];
    used[m] = in && (!prob || a.w[m] != 0.f);
  }
  float* out = a.out + (int64_t)row * a.ldo;
  const int V4 = a.vec ? (V & ~3) : 0;           // columns [0, V4) go four at a time, the rest one at a time

  float lse[KMAX], lw[KMAX];
#pragma unroll
  for (int m = 0; m < KMAX; ++m) lse[m] = lw[m] = 0.f;
  float thr = -INFINITY;
  int best = -1;

  if (cut) {
    for (int w = tid; w < (V + 31) / 32; w += NTHREADS) ban[w] = 0u;
    __syncthreads();
    for (int b = tid; b < a.nbanned; b += NTHREADS) {
      const int id = a.banned[b];
      if (id >= 0 && id < V) atomicOr(&ban[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
  }

  if (prob || cut) {
    float mx[KMAX], sm[KMAX];
#pragma unroll
    for (int m = 0; m < KMAX; ++m) { mx[m] = -INFINITY; sm[m] = 0.f; }
    float bv = -INFINITY;
    int bi = 0x7fffffff;                         // member 0's best eligible id so far (value desc, id asc)
    const int f = (cut && a.flags != nullptr) ? a.flags[row] : 0;
    auto fold = [&](auto wc, int j) {
      constexpr int W = decltype(wc)::value;
#pragma unroll
      for (int m = 0; m < KMAX; ++m) {
        const bool sum = prob && used[m], rank = cut && m == 0;
        if (!sum && !rank) continue;
        float v[W];
        load_w<W>(x[m] + j, v);
        if (sum) {
          float mn = mx[m];
#pragma unroll
          for (int e = 0; e < W; ++e) mn = fmaxf(mn, v[e]);
          if (mn > -INFINITY) {
            float s = sm[m] * expf(mx[m] - mn);
#pragma unroll
            for (int e = 0; e < W; ++e) s = s + expf(v[e] - mn);
            sm[m] = s;
            mx[m] = mn;
          }
        }
        if (rank) {
#pragma unroll
          for (int e = 0; e < W; ++e) {
            const int id = j + e;
            const bool eligible = !((ban[id >> 5] >> (id & 31)) & 1u) && !((f & 1) && id == sep);
            if (eligible && (v[e] > bv || (v[e] == bv && id < bi))) { bv = v[e]; bi = id; }
          }
        }
      }
    };
    for (int j = tid * 4; j < V4; j += NTHREADS * 4) fold(width<4>{}, j);
    for (int j = V4 + tid; j < V; j += NTHREADS) fold(width<1>{}, j);

#pragma unroll
    for (int m = 0; m < KMAX; ++m) {
      if (!(prob && used[m])) continue;
      float M1 = mx[m], s = sm[m];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(M1, o, 64), s2 = __shfl_xor(s, o, 64);
        const float M = fmaxf(M1, m2);
        s = (M == -INFINITY) ? 0.f : s * expf(M1 - M) + s2 * expf(m2 - M);
        M1 = M;
      }
      if (lane == 0) { rm[m][wave] = M1; rs[m][wave] = s; }
    }
    if (cut) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(bv, o, 64);
        const int i2 = __shfl_xor(bi, o, 64);
        if (i2 != 0x7fffffff && (bi == 0x7fffffff || v2 > bv || (v2 == bv && i2 < bi))) { bv = v2; bi = i2; }
      }
      if (lane == 0) { cv[wave] = bv; ci[wave] = bi; }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < KMAX; ++m) {
      if (!(prob && used[m])) continue;
      float M = rm[m][0];
      for (int w = 1; w < NWAVES; ++w) M = fmaxf(M, rm[m][w]);
      float tot = 0.f;
      for (int w = 0; w < NWAVES; ++w)
        if (rm[m][w] > -INFINITY) tot = tot + rs[m][w] * expf(rm[m][w] - M);
      lse[m] = M + logf(tot);
      lw[m] = logf(a.w[m]);
    }
    if (cut) {
      bv = cv[0];
      bi = ci[0];
      for (int w = 1; w < NWAVES; ++w) {
        const float v2 = cv[w];
        const int i2 = ci[w];
        if (i2 != 0x7fffffff && (bi == 0x7fffffff || v2 > bv || (v2 == bv && i2 < bi))) { bv = v2; bi = i2; }
      }
      if (bi != 0x7fffffff) {
        thr = bv + a.log_alpha;
        best = bi;
      }
    }
  }

  auto emit = [&](auto wc, int j) {
    constexpr int W = decltype(wc)::value;
    float v[KMAX][W];
#pragma unroll
    for (int m = 0; m < KMAX; ++m) {
      if (used[m] || (cut && m == 0)) {
        load_w<W>(x[m] + j, v[m]);
      } else {
#pragma unroll
        for (int e = 0; e < W; ++e) v[m][e] = 0.f;
      }
    }
    float z[W];
#pragma unroll
    for (int e = 0; e < W; ++e) {
      if (!prob) {
        float acc = rounded(a.w[0] * v[0][e]);
#pragma unroll
        for (int m = 1; m < KMAX; ++m)
          if (m < a.K) acc = acc + rounded(a.w[m] * v[m][e]);
        z[e] = acc;
      } else {
        float t[KMAX], T = -INFINITY;
#pragma unroll
        for (int m = 0; m < KMAX; ++m) {
          t[m] = (used[m] && v[m][e] > -INFINITY) ? (v[m][e] - lse[m]) + lw[m] : -INFINITY;
          T = fmaxf(T, t[m]);
        }
        if (T > -INFINITY) {
          float s = 0.f;
#pragma unroll
          for (int m = 0; m < KMAX; ++m)
            if (used[m]) s = s + expf(t[m] - T);
          z[e] = T + logf(s);
        } else {
          z[e] = -INFINITY;
        }
      }
      if (cut) {
        const int id = j + e;
        if (id != sep && id != best && v[0][e] < thr) z[e] = -INFINITY;
      }
    }
    store_w<W>(out + j, z);
  };
  for (int j = tid * 4; j < V4; j += NTHREADS * 4) emit(width<4>{}, j);
  for (int j = V4 + tid; j < V; j += NTHREADS) emit(width<1>{}, j);
}

bool aligned16(const void* p, int ld) { return ((uintptr_t)p & 15u) == 0 && (ld & 3) == 0; }

}  // namespace

extern "C" int unimm_mix_version(void) { return 1; }

extern "C" int unimm_lm_mix(const unimm_lm_mix_args* a, void* stream) {
  if (a == nullptr || a->out == nullptr) return UNIMM_E_ARG;
  if (a->K < 1 || a->K > KMAX) return UNIMM_E_ARG;
  if (a->mode != UNIMM_MIX_LOGIT && a->mode != UNIMM_MIX_PROB) return UNIMM_E_ARG;
  if (a->rows < 0 || a->V < 1 || a->V > VMAX || a->ldo < a->V || a->nbanned < 0 || (a->nbanned > 0 && a->banned == nullptr))
    return UNIMM_E_ARG;
  const bool prob = a->mode == UNIMM_MIX_PROB;
  bool any = false, vec = aligned16(a->out, a->ldo);
  for (int m = 0; m < a->K; ++m) {
    const float w = a->w[m];
    if (a->x[m] == nullptr || a->ld[m] < a->V) return UNIMM_E_ARG;
    if (!(w > -INFINITY && w < INFINITY)) return UNIMM_E_ARG;
    if (prob && w < 0.f) return UNIMM_E_ARG;
    any = any || w != 0.f;
    vec = vec && aligned16(a->x[m], a->ld[m]);
  }
  if (prob && !any) return UNIMM_E_ARG;
  if (a->rows == 0) return UNIMM_OK;
  // out against the bounding range of every member's rows
  const uintptr_t o0 = (uintptr_t)a->out, o1 = o0 + ((uintptr_t)(a->rows - 1) * (uintptr_t)a->ldo + (uintptr_t)a->V) * sizeof(float);
  for (int m = 0; m < a->K; ++m) {
    const uintptr_t x0 = (uintptr_t)a->x[m];
    const uintptr_t x1 = x0 + ((uintptr_t)(a->rows - 1) * (uintptr_t)a->ld[m] + (uintptr_t)a->V) * sizeof(float);
    if (o0 < x1 && x0 < o1) return UNIMM_E_ARG;
  }
  MixParams p;
  for (int m = 0; m < KMAX; ++m) {
    const bool in = m < a->K;
    p.x[m] = in ? a->x[m] : nullptr;
    p.ld[m] = in ? a->ld[m] : 0;
    p.w[m] = in ? a->w[m] : 0.f;
  }
  p.out = a->out; p.banned = a->banned; p.flags = a->flags;
  p.K = a->K; p.prob = prob; p.cut = a->log_alpha > -INFINITY; p.vec = vec;
  p.rows = a->rows; p.V = a->V; p.ldo = a->ldo; p.nbanned = a->nbanned; p.sep = a->sep;
  p.log_alpha = a->log_alpha;
  hipLaunchKernelGGL(lm_mix_kernel, dim3((unsigned)p.rows), dim3(NTHREADS), 0, (hipStream_t)stream, p);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}
