// Answer generation kernels (include/unimm_hip.h, ABI 19-20): text self-attention of the decode rows against a shared context
// cache plus per-hypothesis private caches (unimm_attn_verify: its pair-structured form for speculative decoding, with the in-place
// unimm_kv_cache_append), the per-step private-cache append + reorder, log-softmax + top-K of the
// decoder logits (beam search), and temperature / top-k / nucleus sampling from them (unimm_lm_sample, ABI 20; with per-row
// parameters unimm_lm_sample_rows, ABI 24: the same kernel template).  unimm_lm_topk_hist / unimm_lm_sample_hist are the same two
// kernel templates with HIST on: a per-row token history adds no-repeat n-gram bans and a repetition penalty (apply_history).
// unimm_lm_spec_verify is the rejection step of speculative sampling: the sampler's selection on a model row and a draft row.
// unimm_amd/generation.py drives them; the mask argument that makes the cache exact is in its docstring.
#include <math.h>

#include "common.h"

namespace {

constexpr int NTHREADS = 256;
constexpr int DH = 64;          // head size of the text stream
constexpr int QMAX = 32;        // nr * beams query rows per (group, head)
constexpr int KMAX = 320;       // keys per query row: context (<= 256) + private + own new rows (T <= 256 bounds the sum)
constexpr int TOPK_MAX = 16;
constexpr int VMAX = 65536;     // vocabulary bound of the banned-id bitmask

struct DecodeParams {
  const bf16_t *q, *k, *v;
  bf16_t* out;
  const bf16_t *ctx_k, *ctx_v;
  const int32_t *ctx_off, *ctx_len;
  const bf16_t *priv_k, *priv_v;
  const int32_t* plen;
  int G, beams, nr, H, pcap;
  int ldq, ldk, ldv, ldo, ldc, ldp;
  float scale;
};

// 64 bf16 of one key row -> fp32 registers (eight 16-byte loads)
__device__ __forceinline__ void load_row64(const bf16_t* p, float (&f)[DH]) {
  const uint4* p4 = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int c = 0; c < DH / 8; ++c) {
    const uint4 w = p4[c];
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      f[c * 8 + 2 * e] = __uint_as_float(u[e] << 16);
      f[c * 8 + 2 * e + 1] = __uint_as_float(u[e] & 0xffff0000u);
    }
  }
}

__device__ __forceinline__ float dot64(const float* q, const float (&k)[DH]) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    a0 = fmaf(q[d], k[d], a0);
    a1 = fmaf(q[d + 1], k[d + 1], a1);
    a2 = fmaf(q[d + 2], k[d + 2], a2);
    a3 = fmaf(q[d + 3], k[d + 3], a3);
  }
  return (a0 + a1) + (a2 + a3);
}

__global__ __launch_bounds__(NTHREADS) void attn_decode_kernel(DecodeParams p) {
  __shared__ float Qs[QMAX * DH];
  __shared__ float S[QMAX * KMAX];
  const int tid = threadIdx.x;
  const int g = blockIdx.x / p.H, h = blockIdx.x % p.H;
  const int nq = p.beams * p.nr;
  const int row0 = g * nq;                       // first new row of the group
  const int slot0 = g * p.beams;
  const int c = min(max(p.ctx_len[g], 0), 256);
  const int co = p.ctx_off[g];
  // cached rows of slot s, bounded so that every key index stays inside the LDS score row
  auto plen_of = [&](int s) { return min(min(max(p.plen[s], 0), p.pcap), KMAX - p.nr - c); };

  for (int idx = tid; idx < nq * DH; idx += NTHREADS) {
    const int r = idx / DH, d = idx % DH;
    Qs[idx] = bf2f(p.q[(int64_t)(row0 + r) * p.ldq + h * DH + d]) * p.scale;
  }
  __syncthreads();

  // scores against the shared context: one key row per thread, every query row of the group
  for (int j = tid; j < c; j += NTHREADS) {
    float kf[DH];
    load_row64(p.ctx_k + (int64_t)(co + j) * p.ldc + h * DH, kf);
    for (int r = 0; r < nq; ++r) S[r * KMAX + j] = dot64(Qs + r * DH, kf);
  }
  // scores against each slot's private rows, then its own new rows (causal among the new rows)
  const int npk = p.pcap + p.nr;
  for (int t = tid; t < p.beams * npk; t += NTHREADS) {
    const int b = t / npk, j = t % npk;
    const int s = slot0 + b;
    const int pl = plen_of(s);
    if (j >= pl + p.nr) continue;
    float kf[DH];
    if (j < pl)
      load_row64(p.priv_k + ((int64_t)s * p.pcap + j) * p.ldp + h * DH, kf);
    else
      load_row64(p.k + (int64_t)(s * p.nr + (j - pl)) * p.ldk + h * DH, kf);
    for (int i = 0; i < p.nr; ++i)
      if (j < pl || j - pl <= i) S[(b * p.nr + i) * KMAX + c + j] = dot64(Qs + (b * p.nr + i) * DH, kf);
  }
  __syncthreads();

  // softmax of every row over its key prefix [0, c + plen + i + 1): one wave per row
  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < nq; r += NTHREADS / 64) {
    const int b = r / p.nr, i = r % p.nr;
    const int nk = c + plen_of(slot0 + b) + i + 1;
    float* Sr = S + r * KMAX;
    float m = -INFINITY;
    for (int j = lane; j < nk; j += 64) m = fmaxf(m, Sr[j]);
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < nk; j += 64) {
      const float e = expf(Sr[j] - m);
      Sr[j] = e;
      sum += e;
    }
    const float inv = 1.0f / wave_sum(sum);
    for (int j = lane; j < nk; j += 64) Sr[j] *= inv;
  }
  __syncthreads();

  // P.V: thread = (output column d, row group rg); the context V rows are read once per row group
  const int d = tid & (DH - 1), rg = tid >> 6;
  constexpr int RPT = QMAX / (NTHREADS / DH);    // 8 rows per thread
  float acc[RPT];
#pragma unroll
  for (int u = 0; u < RPT; ++u) acc[u] = 0.f;
  // eight V rows in flight per iteration: one dependent load per key left this loop latency-bound (~200 us per launch)
  const bf16_t* vcol = p.ctx_v + (int64_t)co * p.ldc + h * DH + d;
  constexpr int VU = 8;
  int j = 0;
  for (; j + VU <= c; j += VU) {
    float v[VU];
#pragma unroll
    for (int e = 0; e < VU; ++e) v[e] = bf2f(vcol[(int64_t)(j + e) * p.ldc]);
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
      const int r = rg + 4 * u;
      if (r < nq) {
#pragma unroll
        for (int e = 0; e < VU; ++e) acc[u] = fmaf(S[r * KMAX + j + e], v[e], acc[u]);
      }
    }
  }
  for (; j < c; ++j) {
    const float v = bf2f(vcol[(int64_t)j * p.ldc]);
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
      const int r = rg + 4 * u;
      if (r < nq) acc[u] = fmaf(S[r * KMAX + j], v, acc[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < RPT; ++u) {
    const int r = rg + 4 * u;
    if (r >= nq) continue;
    const int b = r / p.nr, i = r % p.nr, s = slot0 + b;
    const int pl = plen_of(s);
    float a = acc[u];
    const bf16_t* pcol = p.priv_v + (int64_t)s * p.pcap * p.ldp + h * DH + d;
    int j = 0;
    for (; j + 4 <= pl; j += 4) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = bf2f(pcol[(int64_t)(j + e) * p.ldp]);
#pragma unroll
      for (int e = 0; e < 4; ++e) a = fmaf(S[r * KMAX + c + j + e], v[e], a);
    }
    for (; j < pl; ++j) a = fmaf(S[r * KMAX + c + j], bf2f(pcol[(int64_t)j * p.ldp]), a);
    for (int e = 0; e <= i; ++e)
      a = fmaf(S[r * KMAX + c + pl + e], bf2f(p.v[(int64_t)(s * p.nr + e) * p.ldv + h * DH + d]), a);
    p.out[(int64_t)(row0 + r) * p.ldo + h * DH + d] = f2bf(a);
  }
}

// Pair-structured form of the kernel above (unimm_attn_verify): the nr new rows of a slot are nr / 2 (answer row, copy row) pairs.
// New row i (pair i / 2, kind i % 2) attends the context, the private rows, the ANSWER rows of the pairs <= its own and, a copy
// row, itself; its keys among the new rows are compacted into score columns [c + pl, c + pl + i / 2 + 1 + i % 2), so the softmax
// and P.V walk a key prefix exactly as above.  Same staging, dot product, lane order and fma chain: nr = 2 gives the same bits.
__global__ __launch_bounds__(NTHREADS) void attn_verify_kernel(DecodeParams p) {
  __shared__ float Qs[QMAX * DH];
  __shared__ float S[QMAX * KMAX];
  const int tid = threadIdx.x;
  const int g = blockIdx.x / p.H, h = blockIdx.x % p.H;
  const int nq = p.beams * p.nr;
  const int row0 = g * nq;
  const int slot0 = g * p.beams;
  const int c = min(max(p.ctx_len[g], 0), 256);
  const int co = p.ctx_off[g];
  auto plen_of = [&](int s) { return min(min(max(p.plen[s], 0), p.pcap), KMAX - p.nr - c); };

  for (int idx = tid; idx < nq * DH; idx += NTHREADS) {
    const int r = idx / DH, d = idx % DH;
    Qs[idx] = bf2f(p.q[(int64_t)(row0 + r) * p.ldq + h * DH + d]) * p.scale;
  }
  __syncthreads();

  for (int j = tid; j < c; j += NTHREADS) {
    float kf[DH];
    load_row64(p.ctx_k + (int64_t)(co + j) * p.ldc + h * DH, kf);
    for (int r = 0; r < nq; ++r) S[r * KMAX + j] = dot64(Qs + r * DH, kf);
  }
  // private rows: every new row of the slot; new answer row of pair e: the rows of pairs >= e, column pl + e; new copy row i:
  // row i alone, column pl + i / 2 + 1
  const int npk = p.pcap + p.nr;
  for (int t = tid; t < p.beams * npk; t += NTHREADS) {
    const int b = t / npk, j = t % npk;
    const int s = slot0 + b;
    const int pl = plen_of(s);
    if (j >= pl + p.nr) continue;
    float kf[DH];
    if (j < pl) {
      load_row64(p.priv_k + ((int64_t)s * p.pcap + j) * p.ldp + h * DH, kf);
      for (int i = 0; i < p.nr; ++i) S[(b * p.nr + i) * KMAX + c + j] = dot64(Qs + (b * p.nr + i) * DH, kf);
    } else {
      const int n = j - pl, e = n >> 1;
      load_row64(p.k + (int64_t)(s * p.nr + n) * p.ldk + h * DH, kf);
      if (n & 1) {
        S[(b * p.nr + n) * KMAX + c + pl + e + 1] = dot64(Qs + (b * p.nr + n) * DH, kf);
      } else {
        for (int i = n; i < p.nr; ++i) S[(b * p.nr + i) * KMAX + c + pl + e] = dot64(Qs + (b * p.nr + i) * DH, kf);
      }
    }
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < nq; r += NTHREADS / 64) {
    const int b = r / p.nr, i = r % p.nr;
    const int nk = c + plen_of(slot0 + b) + (i >> 1) + 1 + (i & 1);
    float* Sr = S + r * KMAX;
    float m = -INFINITY;
    for (int j = lane; j < nk; j += 64) m = fmaxf(m, Sr[j]);
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < nk; j += 64) {
      const float e = expf(Sr[j] - m);
      Sr[j] = e;
      sum += e;
    }
    const float inv = 1.0f / wave_sum(sum);
    for (int j = lane; j < nk; j += 64) Sr[j] *= inv;
  }
  __syncthreads();

  const int d = tid & (DH - 1), rg = tid >> 6;
  constexpr int RPT = QMAX / (NTHREADS / DH);
  float acc[RPT];
#pragma unroll
  for (int u = 0; u < RPT; ++u) acc[u] = 0.f;
  const bf16_t* vcol = p.ctx_v + (int64_t)co * p.ldc + h * DH + d;
  constexpr int VU = 8;
  int j = 0;
  for (; j + VU <= c; j += VU) {
    float v[VU];
#pragma unroll
    for (int e = 0; e < VU; ++e) v[e] = bf2f(vcol[(int64_t)(j + e) * p.ldc]);
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
      const int r = rg + 4 * u;
      if (r < nq) {
#pragma unroll
        for (int e = 0; e < VU; ++e) acc[u] = fmaf(S[r * KMAX + j + e], v[e], acc[u]);
      }
    }
  }
  for (; j < c; ++j) {
    const float v = bf2f(vcol[(int64_t)j * p.ldc]);
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
      const int r = rg + 4 * u;
      if (r < nq) acc[u] = fmaf(S[r * KMAX + j], v, acc[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < RPT; ++u) {
    const int r = rg + 4 * u;
    if (r >= nq) continue;
    const int b = r / p.nr, i = r % p.nr, s = slot0 + b;
    const int pl = plen_of(s);
    float a = acc[u];
    const bf16_t* pcol = p.priv_v + (int64_t)s * p.pcap * p.ldp + h * DH + d;
    int j = 0;
    for (; j + 4 <= pl; j += 4) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = bf2f(pcol[(int64_t)(j + e) * p.ldp]);
#pragma unroll
      for (int e = 0; e < 4; ++e) a = fmaf(S[r * KMAX + c + j + e], v[e], a);
    }
    for (; j < pl; ++j) a = fmaf(S[r * KMAX + c + j], bf2f(pcol[(int64_t)j * p.ldp]), a);
    for (int e = 0; e <= (i >> 1); ++e)            // the answer rows of the pairs up to its own
      a = fmaf(S[r * KMAX + c + pl + e], bf2f(p.v[(int64_t)(s * p.nr + 2 * e) * p.ldv + h * DH + d]), a);
    if (i & 1)                                      // a copy row: itself
      a = fmaf(S[r * KMAX + c + pl + (i >> 1) + 1], bf2f(p.v[(int64_t)(s * p.nr + i) * p.ldv + h * DH + d]), a);
    p.out[(int64_t)(row0 + r) * p.ldo + h * DH + d] = f2bf(a);
  }
}

struct KvAppendParams {
  bf16_t* cache; const bf16_t* nkv;
  const int32_t *count, *plen; int32_t* plen_out;
  int layers, slots, pcap, ldp, width, max_count;
  int64_t nls;
  int ld_new, row_mul, row_step;
};

// grid (slots, layers): rows [plen[s], plen[s] + count[s]) of slot s of layer l <- the slot's new rows j * row_step
__global__ __launch_bounds__(NTHREADS) void kv_append_kernel(KvAppendParams a) {
  const int s = blockIdx.x, l = blockIdx.y;
  const int pl = min(max(a.plen[s], 0), a.pcap);
  const int cnt = min(min(max(a.count[s], 0), a.max_count), a.pcap - pl);
  const int vec = a.width / 8;
  bf16_t* dst = a.cache + (((int64_t)l * a.slots + s) * a.pcap + pl) * a.ldp;
  const bf16_t* nrow = a.nkv + l * a.nls + (int64_t)s * a.row_mul * a.ld_new;
  for (int t = threadIdx.x; t < cnt * vec; t += NTHREADS) {
    const int r = t / vec, c = t % vec;
    reinterpret_cast<uint4*>(dst + (int64_t)r * a.ldp)[c] =
        reinterpret_cast<const uint4*>(nrow + (int64_t)r * a.row_step * a.ld_new)[c];
  }
  if (l == 0 && threadIdx.x == 0) a.plen_out[s] = pl + cnt;
}

struct KvParams {
  const bf16_t* src; bf16_t* dst; const bf16_t* nkv;
  const int32_t *parent, *plen; int32_t* plen_out;
  int layers, slots, pcap, ldp, width;
  int64_t nls;
  int ld_new, row_mul;
};

// grid (slots, layers): slot s of layer l <- rows [0, plen[p]) of parent p, then p's new answer row
__global__ __launch_bounds__(NTHREADS) void kv_update_kernel(KvParams a) {
  const int s = blockIdx.x, l = blockIdx.y;
  const int par = min(max(a.parent[s], 0), a.slots - 1);
  const int pl = min(max(a.plen[par], 0), a.pcap - 1);
  const int vec = a.width / 8;
  const bf16_t* src = a.src + ((int64_t)l * a.slots + par) * a.pcap * a.ldp;
  bf16_t* dst = a.dst + ((int64_t)l * a.slots + s) * a.pcap * a.ldp;
  const bf16_t* nrow = a.nkv + l * a.nls + (int64_t)par * a.row_mul * a.ld_new;
  for (int t = threadIdx.x; t < (pl + 1) * vec; t += NTHREADS) {
    const int r = t / vec, c = t % vec;
    const uint4* from = reinterpret_cast<const uint4*>(r < pl ? src + (int64_t)r * a.ldp : nrow) + c;
    reinterpret_cast<uint4*>(dst + (int64_t)r * a.ldp)[c] = *from;
  }
  if (l == 0 && threadIdx.x == 0) a.plen_out[s] = pl + 1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Per-row history (unimm_lm_topk_hist / unimm_lm_sample_hist, the HIST instantiations).  A row's sources are its answer tokens
// a[0, k) and, optionally, one row of a context table; apply_history ORs the ids the no-repeat n-gram rule bans into the
// launch's `ban` bitmap and, when penalty != 1, marks every id of the sources in `seen`, whose logit then takes part in every
// SELECTION as x' = x > 0 ? x * inv_penalty : x * penalty (the reported log p stays that of x).  Everything read from device
// memory is clamped before it indexes anything: k to [0, ldh], the context index to [0, nctx), its length to [0, ldc].
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int HIST_MAX = 128;   // ldh bound: answer tokens per row
constexpr int CTX_MAX = 256;    // ldc bound: context tokens per row

struct HistParams {
  const int32_t *hist, *hist_len, *ctx, *ctx_len, *ctx_idx;
  int ldh, nctx, ldc, ngram, sep;
  float penalty, inv_penalty;
};

template <bool HIST>
struct HistLds {
  uint32_t seen[VMAX / 32];
  int src[HIST_MAX + CTX_MAX];                  // [0, HIST_MAX): the answer, [HIST_MAX, ..): the context
};
template <>
struct HistLds<false> {};

// x' of an id of the sources.  The product is rounded to fp32 HERE: the empty asm keeps -ffp-contract=fast from fusing it into a
// later subtraction, so that x' is the one correctly rounded multiply the header promises.
__device__ __forceinline__ float penalised(float xv, float penalty, float inv_penalty) {
  float xp = xv > 0.f ? xv * inv_penalty : xv * penalty;
  asm volatile("" : "+v"(xp));
  return xp;
}

// Every thread calls it, after the launch-wide bans are in `ban` (and a barrier); it ends with a barrier.
__device__ void apply_history(const HistParams& h, int row, int V, uint32_t* ban, HistLds<true>& l) {
  const int tid = threadIdx.x;
  const int k = h.hist != nullptr ? min(max(h.hist_len[row], 0), h.ldh) : 0;
  const int32_t* a = h.hist != nullptr ? h.hist + (int64_t)row * h.ldh : nullptr;
  const int32_t* c = nullptr;
  int cl = 0;
  if (h.ctx != nullptr) {
    const int ci = min(max(h.ctx_idx[row], 0), h.nctx - 1);
    cl = min(max(h.ctx_len[ci], 0), h.ldc);
    c = h.ctx + (int64_t)ci * h.ldc;
  }
  const bool pen = h.penalty != 1.f;
  if (pen)
    for (int w = tid; w < (V + 31) / 32; w += NTHREADS) l.seen[w] = 0u;
  for (int i = tid; i < HIST_MAX + CTX_MAX; i += NTHREADS)
    l.src[i] = i < HIST_MAX ? (i < k ? a[i] : 0) : (i - HIST_MAX < cl ? c[i - HIST_MAX] : 0);
  __syncthreads();
  const int n = h.ngram;
  const bool grams = n > 0 && k >= n - 1;        // the answer holds the n - 1 tokens a[k-n+1, k) every window is compared with
  for (int i = tid; i < HIST_MAX + CTX_MAX; i += NTHREADS) {
    const bool ans = i < HIST_MAX;
    const int e = ans ? i : i - HIST_MAX;        // the window ends at s[e], wholly inside its own source
    if (e >= (ans ? k : cl)) continue;
    const int* s = l.src + (ans ? 0 : HIST_MAX);
    const int t = s[e];
    if (t < 0 || t >= V) continue;               // an id outside [0, V) bans nothing (it still compares below, as s[e - d])
    if (pen) atomicOr(&l.seen[t >> 5], 1u << (t & 31));
    if (!grams || e < n - 1 || t == h.sep) continue;
    bool eq = true;
    for (int d = 1; d < n; ++d) eq = eq && s[e - d] == l.src[k - d];
    if (eq) atomicOr(&ban[t >> 5], 1u << (t & 31));
  }
  __syncthreads();
}

struct TopkParams {
  const float* logits; const int32_t* banned; const int32_t* flags;
  float* vals; int32_t* ids; float* lse;
  int rows, V, ldl, nbanned, sep, K;
  HistParams h;                                  // HIST only
};

// (va, ia) ranks before (vb, ib): value desc, id asc
__device__ __forceinline__ bool better(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

// HIST (unimm_lm_topk_hist): the row's history bans join the bitmap, and with a penalty the order is that of x' while the
// reported values stay x - lse; nothing else differs.
template <bool HIST>
__global__ __launch_bounds__(NTHREADS) void lm_topk_kernel(TopkParams a) {
  __shared__ uint32_t ban[VMAX / 32];
  __shared__ HistLds<HIST> hl;
  __shared__ float lv[TOPK_MAX * NTHREADS];
  __shared__ int li[TOPK_MAX * NTHREADS];
  __shared__ float rm[NTHREADS / 64], rs[NTHREADS / 64];
  __shared__ int wi[NTHREADS / 64];
  __shared__ float wv[NTHREADS / 64];
  const int tid = threadIdx.x, row = blockIdx.x;
  const int nw = (a.V + 31) / 32;
  for (int w = tid; w < nw; w += NTHREADS) ban[w] = 0u;
  __syncthreads();
  for (int b = tid; b < a.nbanned; b += NTHREADS) {
    const int id = a.banned[b];
    if (id >= 0 && id < a.V) atomicOr(&ban[id >> 5], 1u << (id & 31));
  }
  __syncthreads();
  bool pen = false;
  if constexpr (HIST) {
    apply_history(a.h, row, a.V, ban, hl);
    pen = a.h.penalty != 1.f;
  }
  const int f = a.flags != nullptr ? a.flags[row] : 0;
  const float* x = a.logits + (int64_t)row * a.ldl;
  const int K = a.K;

  float m = -INFINITY, s = 0.f;
  int n = 0;                                     // entries of this thread's list (value desc, id asc)
  float tv = 0.f;
  int ti = 0;                                    // its last entry once full
  for (int j = tid; j < a.V; j += NTHREADS) {
    const float xv = x[j];
    if (xv > -INFINITY) {
      if (xv > m) {
        s = s * expf(m - xv) + 1.f;
        m = xv;
      } else {
        s += expf(xv - m);
      }
    }
    const bool banned = ((ban[j >> 5] >> (j & 31)) & 1u) || ((f & 1) && j == a.sep) || ((f & 2) && j != a.sep);
    float cv = banned ? -INFINITY : xv;
    if constexpr (HIST) {
      if (pen && !banned && ((hl.seen[j >> 5] >> (j & 31)) & 1u)) cv = penalised(xv, a.h.penalty, a.h.inv_penalty);
    }
    if (n < K || better(cv, j, tv, ti)) {
      int pos = n < K ? n : K - 1;
      while (pos > 0 && better(cv, j, lv[(pos - 1) * NTHREADS + tid], li[(pos - 1) * NTHREADS + tid])) {
        lv[pos * NTHREADS + tid] = lv[(pos - 1) * NTHREADS + tid];
        li[pos * NTHREADS + tid] = li[(pos - 1) * NTHREADS + tid];
        --pos;
      }
      lv[pos * NTHREADS + tid] = cv;
      li[pos * NTHREADS + tid] = j;
      if (n < K) ++n;
      tv = lv[(n - 1) * NTHREADS + tid];
      ti = li[(n - 1) * NTHREADS + tid];
    }
  }

  // log-sum-exp of the row: combine the (max, scaled sum) pairs
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    const float M = fmaxf(m, m2);
    // (lse_combine below restates how this build rounds the next line, for unimm_lm_spec_verify: keep the two in step)
    s = (M == -INFINITY) ? 0.f : s * expf(m - M) + s2 * expf(m2 - M);
    m = M;
  }
  if (lane == 0) { rm[wave] = m; rs[wave] = s; }
  __syncthreads();
  float M = rm[0];
  for (int w = 1; w < NTHREADS / 64; ++w) M = fmaxf(M, rm[w]);
  float tot = 0.f;
  for (int w = 0; w < NTHREADS / 64; ++w)
    if (rm[w] > -INFINITY) tot += rs[w] * expf(rm[w] - M);
  const float lse = M + logf(tot);

  // merge the 256 sorted lists: K rounds of a block-wide arg-best over the list heads
  int hd = 0;
  for (int r = 0; r < K; ++r) {
    float bv = hd < n ? lv[hd * NTHREADS + tid] : -INFINITY;
    int bi = hd < n ? li[hd * NTHREADS + tid] : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(bv, o, 64);
      const int i2 = __shfl_xor(bi, o, 64);
      if (better(v2, i2, bv, bi)) { bv = v2; bi = i2; }
    }
    if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
    __syncthreads();
    bv = wv[0];
    bi = wi[0];
    for (int w = 1; w < NTHREADS / 64; ++w)
      if (better(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
    __syncthreads();
    if (hd < n && li[hd * NTHREADS + tid] == bi) ++hd;
    if (tid == 0) {
      if constexpr (HIST) {                      // ranked by x', reported as the raw log p
        if (pen && bv > -INFINITY && bi >= 0 && bi < a.V) bv = x[bi];
      }
      a.vals[(int64_t)row * K + r] = bv - lse;
      a.ids[(int64_t)row * K + r] = bi;
    }
  }
  if (tid == 0 && a.lse != nullptr) a.lse[row] = lse;
}

// ---------------------------------------------------------------------------------------------------------------------------
// unimm_lm_sample: one workgroup per logits row.  Every id gets a KEY: 0 when it is not eligible (banned, a flag, a logit that
// is not > -inf), otherwise the order-preserving integer image of its fp32 bits (> 0), so that "logit desc, id asc" is "key desc,
// id asc" and every selection below is an exact radix select on integers.  V <= STAGE_MAX: the keys are staged in LDS once and
// every later pass reads LDS; larger V: the passes recompute the key from the (L2-resident) row.  Masses are summed as
// 2^-40 fixed point in 64-bit integers: an integer sum does not depend on the order of the atomics, so a launch is reproducible.
// PER_ROW (unimm_lm_sample_rows): temperature / top_k / top_p come from device arrays indexed by the row, and values the scalar
// entry point refuses on the host make the row return the `nothing eligible` result; nothing else differs.
// HIST (unimm_lm_sample_hist): the history's bans join the bitmap and the key of an id of the sources is built from x', so every
// selection, q and logq are those of the row x'; lse and logp stay those of x.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int STAGE_MAX = 36864;               // 144 KiB of keys + 12.3 KiB of static LDS <= 160 KiB
// HIST adds the 8 KiB `seen` bitmap and 1.5 KiB of sources (HistLds): 12,416 + 9,728 = 22,144 B of static LDS, which leaves
// 163,840 - 22,144 = 141,696 B = 35,424 keys.  34,816 keys (136 KiB: 139,264 + 22,144 = 161,408 B) keep V = 30522 staged.
constexpr int HIST_STAGE_MAX = 34816;
constexpr float FIX_ONE = 1099511627776.f;     // 2^40
static_assert(NTHREADS == 256, "one histogram bin per thread");

struct SampleParams {
  const float* logits; const int32_t* banned; const int32_t* flags; const int32_t* stream;
  int32_t* token; float* logp; float* logq; float* lse;
  int rows, V, ldl, nbanned, sep, top_k;
  float temperature, top_p;
  uint32_t key;
  const float* temp_rows; const int32_t* topk_rows; const float* topp_rows;   // PER_ROW: [rows] each, instead of the scalars
  HistParams h;                                  // HIST only
};

struct SelScratch {
  unsigned long long hist[256], scan[256], tgt, own;
  uint32_t sel;
};

__device__ __forceinline__ uint32_t ord_key(float x) {
  uint32_t u = __float_as_uint(x);
  if ((u << 1) == 0u) u = 0u;                  // -0 ties +0, as the float comparison of lm_topk has it
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_val(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// The largest w (top_shift + 8 bits wide) with sum{wt_j : active j, w_j >= w} >= target, by 8-bit digits from the top:
// f(j, w, wt) -> active.  *rem = target minus the weight strictly above w, *at = the weight at w.  Every thread calls it.
template <class F>
__device__ uint32_t radix_select(F f, int V, int top_shift, unsigned long long target, SelScratch& s, unsigned long long* rem,
                                 unsigned long long* at) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0u, pmask = 0u;
  unsigned long long own_sel = 0ull;
  for (int shift = top_shift; shift >= 0; shift -= 8) {
    s.hist[tid] = 0ull;
    if (tid == 0) { s.sel = 0u; s.tgt = target; s.own = 0ull; }
    __syncthreads();
    for (int j = tid; j < V; j += NTHREADS) {
      uint32_t w;
      unsigned long long wt;
      if (f(j, w, wt) && (w & pmask) == prefix) atomicAdd(&s.hist[(w >> shift) & 255u], wt);
    }
    __syncthreads();
    const unsigned long long own = s.hist[tid];
    unsigned long long v = own;                  // -> weight of the digits >= tid
    for (int o = 1; o < 256; o <<= 1) {
      s.scan[tid] = v;
      __syncthreads();
      if (tid + o < 256) v += s.scan[tid + o];
      __syncthreads();
    }
    if (v - own < target && target <= v) { s.sel = (uint32_t)tid; s.tgt = target - (v - own); s.own = own; }
    __syncthreads();
    prefix |= s.sel << shift;
    pmask |= 255u << shift;
    target = s.tgt;
    own_sel = s.own;
    __syncthreads();
  }
  *rem = target;
  *at = own_sel;
  return prefix;
}

__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v, unsigned long long* sh) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  unsigned long long t = 0ull;
  for (int w = 0; w < NTHREADS / 64; ++w) t += sh[w];
  return t;
}

template <bool STAGED, bool PER_ROW, bool HIST>
__global__ __launch_bounds__(NTHREADS) void lm_sample_kernel(SampleParams a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint32_t* keys = reinterpret_cast<uint32_t*>(smem);          // [V] when STAGED (no dynamic LDS otherwise)
  __shared__ uint32_t ban[VMAX / 32];
  __shared__ HistLds<HIST> hl;
  __shared__ SelScratch sel;
  __shared__ float rm[NTHREADS / 64], rs[NTHREADS / 64], wv[NTHREADS / 64];
  __shared__ int wi[NTHREADS / 64];
  __shared__ unsigned long long r64[NTHREADS / 64];
  const int tid = threadIdx.x, row = blockIdx.x;
  const int V = a.V;
  const int nw = (V + 31) / 32;
  for (int w = tid; w < nw; w += NTHREADS) ban[w] = 0u;
  __syncthreads();
  for (int b = tid; b < a.nbanned; b += NTHREADS) {
    const int id = a.banned[b];
    if (id >= 0 && id < V) atomicOr(&ban[id >> 5], 1u << (id & 31));
  }
  __syncthreads();
  bool pen = false;
  if constexpr (HIST) {
    apply_history(a.h, row, V, ban, hl);
    pen = a.h.penalty != 1.f;
  }
  const int f = a.flags != nullptr ? a.flags[row] : 0;
  const float* x = a.logits + (int64_t)row * a.ldl;
  const int sep = a.sep;
  // PER_ROW (unimm_lm_sample_rows): the row's own decoding parameters; the arithmetic below is the scalar kernel's
  const float temp = PER_ROW ? a.temp_rows[row] : a.temperature;
  const int top_k = PER_ROW ? a.topk_rows[row] : a.top_k;
  const float top_p = PER_ROW ? a.topp_rows[row] : a.top_p;
  const bool bad = PER_ROW && (!(temp > 0.f) || !(temp < INFINITY) || !(top_p > 0.f && top_p <= 1.f) || top_k < 0);
  // the logit an id is SELECTED by: x' for an id of the sources under a penalty (HIST), the raw logit otherwise
  auto sel_val = [&](int j, float xv) -> float {
    if constexpr (HIST) {
      if (pen && ((hl.seen[j >> 5] >> (j & 31)) & 1u)) return penalised(xv, a.h.penalty, a.h.inv_penalty);
    }
    return xv;
  };
  auto make_key = [&](int j, float xv) -> uint32_t {
    const bool out = ((ban[j >> 5] >> (j & 31)) & 1u) || ((f & 1) && j == sep) || ((f & 2) && j != sep) || !(xv > -INFINITY);
    return out ? 0u : ord_key(sel_val(j, xv));
  };
  auto key_at = [&](int j) -> uint32_t { return STAGED ? keys[j] : make_key(j, x[j]); };

  // pass A: the row's log-sum-exp (lm_topk's online form, the same order of operations), the keys, their count and maximum
  float m = -INFINITY, s = 0.f;
  uint32_t kmax = 0u;
  unsigned long long cnt = 0ull;
  for (int j = tid; j < V; j += NTHREADS) {
    const float xv = x[j];
    if (xv > -INFINITY) {
      if (xv > m) {
        s = s * expf(m - xv) + 1.f;
        m = xv;
      } else {
        s += expf(xv - m);
      }
    }
    const uint32_t k = make_key(j, xv);
    if (STAGED) keys[j] = k;
    kmax = max(kmax, k);
    cnt += k != 0u;
  }
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    const float M = fmaxf(m, m2);
    // (lse_combine below restates how this build rounds the next line, for unimm_lm_spec_verify: keep the two in step)
    s = (M == -INFINITY) ? 0.f : s * expf(m - M) + s2 * expf(m2 - M);
    m = M;
    kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o, 64));
  }
  if (lane == 0) { rm[wave] = m; rs[wave] = s; wi[wave] = (int)kmax; }
  __syncthreads();
  float M = rm[0];
  kmax = (uint32_t)wi[0];
  for (int w = 1; w < NTHREADS / 64; ++w) {
    M = fmaxf(M, rm[w]);
    kmax = max(kmax, (uint32_t)wi[w]);
  }
  float tot = 0.f;
  for (int w = 0; w < NTHREADS / 64; ++w)
    if (rm[w] > -INFINITY) tot += rs[w] * expf(rm[w] - M);
  const float lse = M + logf(tot);
  cnt = block_sum_u64(cnt, r64);                 // (its barriers also order the key stores before the passes below)
  if (tid == 0 && a.lse != nullptr) a.lse[row] = lse;
  if (cnt == 0ull || bad) {                      // nothing eligible, or (PER_ROW) parameters the host could not refuse
    if (tid == 0) {
      a.token[row] = -1;
      a.logp[row] = -INFINITY;
      a.logq[row] = -INFINITY;
    }
    return;
  }

  // top-k: key T of rank top_k and, where the ids tied at T do not all fit, the last id that does
  uint32_t T = 0u;
  int idcut = -1;                                // kept by top-k: key > T, or key == T and id <= idcut
  if (top_k > 0 && (unsigned long long)top_k < cnt) {
    unsigned long long rem, at;
    T = radix_select([&](int j, uint32_t& w, unsigned long long& wt) { w = key_at(j); wt = 1ull; return w != 0u; }, V, 24,
                     (unsigned long long)top_k, sel, &rem, &at);
    idcut = V;
    if (rem < at) {
      unsigned long long r2, a2;
      idcut = 0xFFFF - (int)radix_select([&](int j, uint32_t& w, unsigned long long& wt) {
                                           w = 0xFFFFu - (uint32_t)j; wt = 1ull; return key_at(j) == T; },
                                         V, 8, rem, sel, &r2, &a2);
    }
  }
  auto kept_k = [&](int j, uint32_t k) -> bool { return k > T || (k == T && j <= idcut); };

  // temperature: every y is taken relative to the row's largest eligible logit (always kept), y_i - y_max = (x_i - x_max) / t:
  // argmax (y + g), q and logq do not change, and the rounding no longer grows with an offset of the whole row
  const float xmax = key_val(kmax);
  auto rel = [&](uint32_t k) -> float { return (key_val(k) - xmax) / temp; };
  auto fixed = [&](float d) -> unsigned long long { return (unsigned long long)(expf(d) * FIX_ONE); };

  // nucleus: the largest key TH whose mass from the top reaches top_p of the kept mass
  uint32_t TH = 0u;
  if (top_p < 1.0f && cnt > 1ull) {
    unsigned long long z = 0ull;
    for (int j = tid; j < V; j += NTHREADS) {
      const uint32_t k = key_at(j);
      if (kept_k(j, k)) z += fixed(rel(k));
    }
    z = block_sum_u64(z, r64);
    const double want = ceil((double)top_p * (double)z);
    const unsigned long long target = want < 1.0 ? 1ull : (unsigned long long)want;
    unsigned long long rem, at;
    TH = radix_select([&](int j, uint32_t& w, unsigned long long& wt) {
                        w = key_at(j);
                        const bool on = kept_k(j, w);
                        wt = on ? fixed(rel(w)) : 0ull;
                        return on; },
                      V, 24, target, sel, &rem, &at);
  }

  // draw: argmax of y + Gumbel noise over the kept ids (ties to the smaller id), and the kept mass
  const uint32_t sk = mix32(a.key ^ ((uint32_t)a.stream[row] * 0x9E3779B1u + 0x7F4A7C15u));
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  unsigned long long zf = 0ull;
  for (int j = tid; j < V; j += NTHREADS) {
    const uint32_t k = key_at(j);
    if (!kept_k(j, k) || k < TH) continue;
    const float d = rel(k);
    zf += fixed(d);
    const uint32_t h = mix32(sk + (uint32_t)j * 0x85EBCA77u);
    const float u = ((float)(h >> 9) + 0.5f) * 1.1920928955078125e-07f;      // 2^-23: exact, inside (0, 1)
    const float v = d - logf(-logf(u));
    if (better(v, j, bv, bi)) { bv = v; bi = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(bv, o, 64);
    const int i2 = __shfl_xor(bi, o, 64);
    if (better(v2, i2, bv, bi)) { bv = v2; bi = i2; }
  }
  if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
  zf = block_sum_u64(zf, r64);                   // (its barriers publish wv / wi)
  if (tid == 0) {
    bv = wv[0];
    bi = wi[0];
    for (int w = 1; w < NTHREADS / 64; ++w)
      if (better(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
    if (bi < 0 || bi >= V) {                     // cannot happen (the top-ranked id is always kept); never index with it
      a.token[row] = -1;
      a.logp[row] = -INFINITY;
      a.logq[row] = -INFINITY;
    } else {
      const float xt = x[bi];
      a.token[row] = bi;
      a.logp[row] = xt - lse;
      a.logq[row] = (sel_val(bi, xt) - xmax) / temp - logf((float)((double)zf * 9.094947017729282e-13));   // 2^-40
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// unimm_lm_spec_verify: the rejection step of speculative sampling, one workgroup per (model row x, draft row xd, draft token d).
// P~ and Q~ are lm_sample_kernel<., PER_ROW>'s distributions of x and of xd.  row_select below is that kernel's passes up to the
// draw, statement for statement (lm_sample_kernel keeps its own inline copy so that its instruction stream does not move); it
// returns the kept set as a DESCRIPTOR: id j with key k is kept iff k > T or (k == T and j <= idcut), and k >= TH; its
// log-probability is (key_val(k) - xmax) / t - lz.  The kernel runs it on xd first (keys staged in LDS when V <= STAGE_MAX),
// keeps Q~'s descriptor in registers, runs it again on x over the same LDS, and then makes ONE pass over P~'s kept ids that
// reads xd_j from global memory against Q~'s descriptor: x is read once, xd twice.  A row without a draft skips the xd phase.
// ---------------------------------------------------------------------------------------------------------------------------
struct SpecParams {
  const float *x, *xd;
  const int32_t *draft, *banned, *flags, *stream;
  const float* temp_rows; const int32_t* topk_rows; const float* topp_rows;
  int32_t *accept, *token;
  float *logp, *logq, *lse, *log_ratio;
  int rows, V, ldl, ldd, nbanned, sep;
  uint32_t key_accept, key_residual;
};

struct RowSel {
  unsigned long long cnt;                        // eligible ids; 0: nothing below is defined
  uint32_t T, TH, kmax;
  int idcut;
  float xmax, lz, lse;                           // lz = logf of the kept mass relative to exp(0) at xmax; lse: LSE only
  __device__ __forceinline__ bool kept(int j, uint32_t k) const { return (k > T || (k == T && j <= idcut)) && k >= TH && k != 0u; }
};

struct SelLds {
  SelScratch sel;
  float rm[NTHREADS / 64], rs[NTHREADS / 64];
  int wi[NTHREADS / 64];
  unsigned long long r64[NTHREADS / 64];
};

// s * e + s2 * e2 of the log-sum-exp's butterfly, ROUNDED AS lm_topk_kernel / lm_sample_kernel round it.  Those kernels leave the
// expression to -ffp-contract=fast, and their build fuses it as fma(s, e, s2 * e2) in the rounds o = 32 .. 2 and evaluates the
// last round (o = 1) as two rounded products and a sum; lse must equal theirs bit for bit (property (i) of the header), so the
// choice is spelled out here instead of being left to the compiler a second time.  tests/test_gpu_spec_sample_edges.py compares
// lse with both kernels on every row.
__device__ __forceinline__ float lse_combine(float s, float e, float s2, float e2, bool fused) {
#pragma clang fp contract(off)
  const float a = s * e, b = s2 * e2;
  return fused ? fmaf(s, e, b) : a + b;
}

// Every thread calls it.  LSE: also the log-sum-exp of x[0:V] (lm_topk's online form).  stop: return after the first pass
// with cnt = 0 (a row whose parameters the host could not refuse still reports its lse).
template <bool STAGED, bool LSE>
__device__ RowSel row_select(const float* x, int V, const uint32_t* ban, int f, int sep, float temp, int top_k, float top_p,
                             bool stop, uint32_t* keys, SelLds& l) {
  const int tid = threadIdx.x;
  auto make_key = [&](int j, float xv) -> uint32_t {
    const bool out = ((ban[j >> 5] >> (j & 31)) & 1u) || ((f & 1) && j == sep) || ((f & 2) && j != sep) || !(xv > -INFINITY);
    return out ? 0u : ord_key(xv);
  };
  auto key_at = [&](int j) -> uint32_t { return STAGED ? keys[j] : make_key(j, x[j]); };
  RowSel r;
  r.T = 0u; r.TH = 0u; r.idcut = -1; r.xmax = 0.f; r.lz = 0.f; r.lse = 0.f;

  float m = -INFINITY, s = 0.f;
  uint32_t kmax = 0u;
  unsigned long long cnt = 0ull;
  __syncthreads();                               // the keys of an earlier call are no longer read
  for (int j = tid; j < V; j += NTHREADS) {
    const float xv = x[j];
    if (LSE && xv > -INFINITY) {
      if (xv > m) {
        s = s * expf(m - xv) + 1.f;
        m = xv;
      } else {
        s += expf(xv - m);
      }
    }
    const uint32_t k = make_key(j, xv);
    if (STAGED) keys[j] = k;
    kmax = max(kmax, k);
    cnt += k != 0u;
  }
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    if (LSE) {
      const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
      const float M = fmaxf(m, m2);
      s = (M == -INFINITY) ? 0.f : lse_combine(s, expf(m - M), s2, expf(m2 - M), o > 1);
      m = M;
    }
    kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o, 64));
  }
  if (lane == 0) { l.rm[wave] = m; l.rs[wave] = s; l.wi[wave] = (int)kmax; }
  __syncthreads();
  float M = l.rm[0];
  kmax = (uint32_t)l.wi[0];
  for (int w = 1; w < NTHREADS / 64; ++w) {
    M = fmaxf(M, l.rm[w]);
    kmax = max(kmax, (uint32_t)l.wi[w]);
  }
  if (LSE) {
    float tot = 0.f;
    for (int w = 0; w < NTHREADS / 64; ++w)
      if (l.rm[w] > -INFINITY) tot += l.rs[w] * expf(l.rm[w] - M);
    r.lse = M + logf(tot);
  }
  cnt = block_sum_u64(cnt, l.r64);
  r.cnt = stop ? 0ull : cnt;
  r.kmax = kmax;
  if (r.cnt == 0ull) return r;

  if (top_k > 0 && (unsigned long long)top_k < cnt) {
    unsigned long long rem, at;
    r.T = radix_select([&](int j, uint32_t& w, unsigned long long& wt) { w = key_at(j); wt = 1ull; return w != 0u; }, V, 24,
                       (unsigned long long)top_k, l.sel, &rem, &at);
    r.idcut = V;
    if (rem < at) {
      const uint32_t T = r.T;
      unsigned long long r2, a2;
      r.idcut = 0xFFFF - (int)radix_select([&](int j, uint32_t& w, unsigned long long& wt) {
                                             w = 0xFFFFu - (uint32_t)j; wt = 1ull; return key_at(j) == T; },
                                           V, 8, rem, l.sel, &r2, &a2);
    }
  }
  const uint32_t T = r.T;
  const int idcut = r.idcut;
  auto kept_k = [&](int j, uint32_t k) -> bool { return k > T || (k == T && j <= idcut); };
  const float xmax = key_val(kmax);
  r.xmax = xmax;
  auto rel = [&](uint32_t k) -> float { return (key_val(k) - xmax) / temp; };
  auto fixed = [&](float d) -> unsigned long long { return (unsigned long long)(expf(d) * FIX_ONE); };

  if (top_p < 1.0f && cnt > 1ull) {
    unsigned long long z = 0ull;
    for (int j = tid; j < V; j += NTHREADS) {
      const uint32_t k = key_at(j);
      if (kept_k(j, k)) z += fixed(rel(k));
    }
    z = block_sum_u64(z, l.r64);
    const double want = ceil((double)top_p * (double)z);
    const unsigned long long target = want < 1.0 ? 1ull : (unsigned long long)want;
    unsigned long long rem, at;
    r.TH = radix_select([&](int j, uint32_t& w, unsigned long long& wt) {
                          w = key_at(j);
                          const bool on = kept_k(j, w);
                          wt = on ? fixed(rel(w)) : 0ull;
                          return on; },
                        V, 24, target, l.sel, &rem, &at);
  }
  unsigned long long zf = 0ull;
  for (int j = tid; j < V; j += NTHREADS) {
    const uint32_t k = key_at(j);
    if (r.kept(j, k)) zf += fixed(rel(k));
  }
  zf = block_sum_u64(zf, l.r64);
  r.lz = logf((float)((double)zf * 9.094947017729282e-13));                    // 2^-40
  return r;
}

template <bool STAGED>
__global__ __launch_bounds__(NTHREADS) void lm_spec_verify_kernel(SpecParams a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint32_t* keys = reinterpret_cast<uint32_t*>(smem);          // [V] when STAGED: xd's keys, then x's
  __shared__ uint32_t ban[VMAX / 32];
  __shared__ SelLds l;
  __shared__ float wv[NTHREADS / 64];
  __shared__ int wb[NTHREADS / 64], wf[NTHREADS / 64];
  const int tid = threadIdx.x, row = blockIdx.x;
  const int V = a.V;
  const int nw = (V + 31) / 32;
  for (int w = tid; w < nw; w += NTHREADS) ban[w] = 0u;
  __syncthreads();
  for (int b = tid; b < a.nbanned; b += NTHREADS) {
    const int id = a.banned[b];
    if (id >= 0 && id < V) atomicOr(&ban[id >> 5], 1u << (id & 31));
  }
  __syncthreads();
  const int f = a.flags != nullptr ? a.flags[row] : 0;
  const float* x = a.x + (int64_t)row * a.ldl;
  const float* xd = a.xd + (int64_t)row * a.ldd;
  const int sep = a.sep;
  const int d = a.draft[row];
  const float temp = a.temp_rows[row];
  const int top_k = a.topk_rows[row];
  const float top_p = a.topp_rows[row];
  const bool bad = !(temp > 0.f) || !(temp < INFINITY) || !(top_p > 0.f && top_p <= 1.f) || top_k < 0;
  auto make_key = [&](int j, float xv) -> uint32_t {
    const bool out = ((ban[j >> 5] >> (j & 31)) & 1u) || ((f & 1) && j == sep) || ((f & 2) && j != sep) || !(xv > -INFINITY);
    return out ? 0u : ord_key(xv);
  };

  RowSel q = {};                                 // no draft (d = -1), or nothing eligible in xd: K_Q is empty
  if (d != -1 && !bad) q = row_select<STAGED, false>(xd, V, ban, f, sep, temp, top_k, top_p, false, keys, l);
  const bool has_q = q.cnt != 0ull;
  const RowSel p = row_select<STAGED, true>(x, V, ban, f, sep, temp, top_k, top_p, bad, keys, l);
  if (p.cnt == 0ull) {                           // nothing eligible, or parameters the host could not refuse
    if (tid == 0) {
      a.lse[row] = p.lse;
      a.token[row] = -1;
      a.accept[row] = 0;
      a.logp[row] = -INFINITY;
      a.logq[row] = -INFINITY;
      if (a.log_ratio != nullptr) a.log_ratio[row] = -INFINITY;
    }
    return;
  }
  auto key_p = [&](int j) -> uint32_t { return STAGED ? keys[j] : make_key(j, x[j]); };
  auto log_p = [&](uint32_t k) -> float { return (key_val(k) - p.xmax) / temp - p.lz; };
  auto log_q = [&](uint32_t k) -> float { return (key_val(k) - q.xmax) / temp - q.lz; };

  // the residual draw: Gumbel-max on y + log(1 - Q~/P~) over K_P; and the first id of P~'s rank order, the fallback
  const uint32_t sk = mix32(a.key_residual ^ ((uint32_t)a.stream[row] * 0x9E3779B1u + 0x7F4A7C15u));
  float bv = -INFINITY;
  int bi = 0x7fffffff, fi = 0x7fffffff;
  for (int j = tid; j < V; j += NTHREADS) {
    const uint32_t k = key_p(j);
    if (!p.kept(j, k)) continue;
    if (k == p.kmax) fi = min(fi, j);
    const float y = (key_val(k) - p.xmax) / temp;
    float l1 = 0.f;
    if (has_q) {
      const uint32_t kq = make_key(j, xd[j]);
      if (q.kept(j, kq)) {
        const float rho = expf(log_q(kq) - (y - p.lz));
        if (!(rho < 1.f)) continue;
        l1 = log1pf(-rho);
      }
    }
    const uint32_t h = mix32(sk + (uint32_t)j * 0x85EBCA77u);
    const float u = ((float)(h >> 9) + 0.5f) * 1.1920928955078125e-07f;        // 2^-23
    const float v = (y + l1) - logf(-logf(u));
    if (better(v, j, bv, bi)) { bv = v; bi = j; }
  }
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(bv, o, 64);
    const int i2 = __shfl_xor(bi, o, 64);
    if (better(v2, i2, bv, bi)) { bv = v2; bi = i2; }
    fi = min(fi, __shfl_xor(fi, o, 64));
  }
  if (lane == 0) { wv[wave] = bv; wb[wave] = bi; wf[wave] = fi; }
  __syncthreads();
  if (tid != 0) return;
  bv = wv[0];
  bi = wb[0];
  fi = wf[0];
  for (int w = 1; w < NTHREADS / 64; ++w) {
    if (better(wv[w], wb[w], bv, bi)) { bv = wv[w]; bi = wb[w]; }
    fi = min(fi, wf[w]);
  }
  // the acceptance ratio of d
  float ratio = -INFINITY;
  if (d >= 0 && d < V) {
    const uint32_t kd = key_p(d);
    if (p.kept(d, kd)) {
      ratio = INFINITY;
      if (has_q) {
        const uint32_t kq = make_key(d, xd[d]);
        if (q.kept(d, kq)) ratio = log_p(kd) - log_q(kq);
      }
    }
  }
  const uint32_t ha = mix32(mix32(a.key_accept ^ ((uint32_t)a.stream[row] * 0x9E3779B1u + 0x7F4A7C15u)));
  const float ua = ((float)(ha >> 9) + 0.5f) * 1.1920928955078125e-07f;
  const bool acc = logf(ua) < ratio;
  int tok = acc ? d : (bi >= 0 && bi < V ? bi : fi);
  a.lse[row] = p.lse;
  a.accept[row] = acc ? 1 : 0;
  if (a.log_ratio != nullptr) a.log_ratio[row] = ratio;
  if (tok < 0 || tok >= V) {                     // cannot happen (the top-ranked id is always in K_P); never index with it
    a.token[row] = -1;
    a.accept[row] = 0;
    a.logp[row] = -INFINITY;
    a.logq[row] = -INFINITY;
  } else {
    const float xt = x[tok];
    a.token[row] = tok;
    a.logp[row] = xt - p.lse;
    a.logq[row] = (xt - p.xmax) / temp - p.lz;
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

// the checks and the launch of the two decode-attention entry points: they differ in the admitted nr and in the kernel
static int launch_decode(const unimm_attn_decode_args* a, void* stream, bool pairs) {
  if (a == nullptr || a->q == nullptr || a->k == nullptr || a->v == nullptr || a->out == nullptr || a->ctx_k == nullptr ||
      a->ctx_v == nullptr || a->ctx_off == nullptr || a->ctx_len == nullptr || a->plen == nullptr)
    return UNIMM_E_ARG;
  if (a->pcap > 0 && (a->priv_k == nullptr || a->priv_v == nullptr)) return UNIMM_E_ARG;
  if (a->D != DH || a->H < 1 || a->H * DH > 1024 || a->G < 1 || a->beams < 1 ||
      (pairs ? (a->nr < 2 || a->nr > QMAX || a->nr % 2 != 0) : (a->nr != 1 && a->nr != 2)) || a->beams * a->nr > QMAX || a->pcap < 0)
    return UNIMM_E_SHAPE;
  if (!al16(a->q) || !al16(a->k) || !al16(a->v) || !al16(a->ctx_k) || !al16(a->ctx_v) ||
      (a->pcap > 0 && (!al16(a->priv_k) || !al16(a->priv_v) || a->ldp % 8)) ||
      a->ldq % 8 || a->ldk % 8 || a->ldv % 8 || a->ldc % 8)
    return UNIMM_E_ALIGN;
  DecodeParams p;
  p.q = (const bf16_t*)a->q; p.k = (const bf16_t*)a->k; p.v = (const bf16_t*)a->v; p.out = (bf16_t*)a->out;
  p.ctx_k = (const bf16_t*)a->ctx_k; p.ctx_v = (const bf16_t*)a->ctx_v; p.ctx_off = a->ctx_off; p.ctx_len = a->ctx_len;
  p.priv_k = (const bf16_t*)a->priv_k; p.priv_v = (const bf16_t*)a->priv_v; p.plen = a->plen;
  p.G = a->G; p.beams = a->beams; p.nr = a->nr; p.H = a->H; p.pcap = a->pcap;
  p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo; p.ldc = a->ldc; p.ldp = a->ldp;
  p.scale = a->scale;
  if (pairs)
    hipLaunchKernelGGL(attn_verify_kernel, dim3((unsigned)(a->G * a->H)), dim3(NTHREADS), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(attn_decode_kernel, dim3((unsigned)(a->G * a->H)), dim3(NTHREADS), 0, (hipStream_t)stream, p);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

extern "C" int unimm_attn_decode(const unimm_attn_decode_args* a, void* stream) { return launch_decode(a, stream, false); }

extern "C" int unimm_attn_verify(const unimm_attn_decode_args* a, void* stream) { return launch_decode(a, stream, true); }

extern "C" int unimm_kv_cache_append(const unimm_kv_append_args* a, void* stream) {
  if (a == nullptr || a->cache == nullptr || a->new_kv == nullptr || a->count == nullptr || a->plen == nullptr ||
      a->plen_out == nullptr)
    return UNIMM_E_ARG;
  if (a->layers < 1 || a->slots < 1 || a->pcap < 1 || a->width < 8 || a->width > a->ldp || a->max_count < 0 ||
      a->new_row_mul < 0 || a->new_row_step < 0)
    return UNIMM_E_SHAPE;
  if (a->plen == a->plen_out) return UNIMM_E_ARG;
  if (!al16(a->cache) || !al16(a->new_kv) || a->width % 8 || a->ldp % 8 || a->ld_new % 8 || a->new_layer_stride % 8)
    return UNIMM_E_ALIGN;
  KvAppendParams p;
  p.cache = (bf16_t*)a->cache; p.nkv = (const bf16_t*)a->new_kv;
  p.count = a->count; p.plen = a->plen; p.plen_out = a->plen_out;
  p.layers = a->layers; p.slots = a->slots; p.pcap = a->pcap; p.ldp = a->ldp; p.width = a->width; p.max_count = a->max_count;
  p.nls = a->new_layer_stride; p.ld_new = a->ld_new; p.row_mul = a->new_row_mul; p.row_step = a->new_row_step;
  hipLaunchKernelGGL(kv_append_kernel, dim3((unsigned)a->slots, (unsigned)a->layers), dim3(NTHREADS), 0, (hipStream_t)stream, p);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

extern "C" int unimm_kv_cache_update(const unimm_kv_update_args* a, void* stream) {
  if (a == nullptr || a->src == nullptr || a->dst == nullptr || a->new_kv == nullptr || a->parent == nullptr ||
      a->plen == nullptr || a->plen_out == nullptr)
    return UNIMM_E_ARG;
  if (a->layers < 1 || a->slots < 1 || a->pcap < 1 || a->width < 8 || a->width > a->ldp || a->new_row_mul < 1)
    return UNIMM_E_SHAPE;
  if (a->src == a->dst || a->plen == a->plen_out) return UNIMM_E_ARG;
  if (!al16(a->src) || !al16(a->dst) || !al16(a->new_kv) || a->width % 8 || a->ldp % 8 || a->ld_new % 8 ||
      a->new_layer_stride % 8)
    return UNIMM_E_ALIGN;
  KvParams p;
  p.src = (const bf16_t*)a->src; p.dst = (bf16_t*)a->dst; p.nkv = (const bf16_t*)a->new_kv;
  p.parent = a->parent; p.plen = a->plen; p.plen_out = a->plen_out;
  p.layers = a->layers; p.slots = a->slots; p.pcap = a->pcap; p.ldp = a->ldp; p.width = a->width;
  p.nls = a->new_layer_stride; p.ld_new = a->ld_new; p.row_mul = a->new_row_mul;
  hipLaunchKernelGGL(kv_update_kernel, dim3((unsigned)a->slots, (unsigned)a->layers), dim3(NTHREADS), 0, (hipStream_t)stream, p);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

extern "C" int unimm_lm_topk(const float* logits, int32_t rows, int32_t V, int32_t ldl, const int32_t* banned, int32_t nbanned,
                             const int32_t* flags, int32_t sep, int32_t K, float* vals, int32_t* ids, float* lse, void* stream) {
  if (logits == nullptr || vals == nullptr || ids == nullptr || (nbanned > 0 && banned == nullptr)) return UNIMM_E_ARG;
  if (rows < 0 || V < 1 || V > VMAX || ldl < V || K < 1 || K > TOPK_MAX || K > V || nbanned < 0) return UNIMM_E_SHAPE;
  if (rows == 0) return UNIMM_OK;
  TopkParams p;
  p.logits = logits; p.banned = banned; p.flags = flags; p.vals = vals; p.ids = ids; p.lse = lse;
  p.rows = rows; p.V = V; p.ldl = ldl; p.nbanned = nbanned; p.sep = sep; p.K = K;
  p.h = HistParams{};
  hipLaunchKernelGGL(lm_topk_kernel<false>, dim3((unsigned)rows), dim3(NTHREADS), 0, (hipStream_t)stream, p);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

namespace {

template <bool PER_ROW, bool HIST>
int launch_lm_sample(const SampleParams& p, hipStream_t stream) {
  constexpr int BOUND = HIST ? HIST_STAGE_MAX : STAGE_MAX;
  if (p.V <= BOUND) {
    static bool done = false;                    // one per instantiation
    if (!done) {
      if (hipFuncSetAttribute((const void*)lm_sample_kernel<true, PER_ROW, HIST>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              BOUND * (int)sizeof(uint32_t)) != hipSuccess)
        return UNIMM_E_HIP;
      done = true;
    }
    hipLaunchKernelGGL((lm_sample_kernel<true, PER_ROW, HIST>), dim3((unsigned)p.rows), dim3(NTHREADS),
                       (size_t)p.V * sizeof(uint32_t), stream, p);
  } else {
    hipLaunchKernelGGL((lm_sample_kernel<false, PER_ROW, HIST>), dim3((unsigned)p.rows), dim3(NTHREADS), 0, stream, p);
  }
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

// The refusals of a history (before any launch) -> UNIMM_OK and the kernels' form of it
int read_history(const unimm_lm_history* h, HistParams* out) {
  if (h == nullptr) return UNIMM_E_ARG;
  if (!(h->penalty > 0.f) || !(h->penalty < INFINITY) || !(h->inv_penalty > 0.f) || !(h->inv_penalty < INFINITY)) return UNIMM_E_ARG;
  if (h->ngram < 0 || h->ngram > 8) return UNIMM_E_SHAPE;
  if (h->hist == nullptr && (h->ngram > 0 || h->penalty != 1.f)) return UNIMM_E_ARG;
  if (h->hist != nullptr && h->hist_len == nullptr) return UNIMM_E_ARG;
  if (h->hist != nullptr && (h->ldh < 0 || h->ldh > HIST_MAX)) return UNIMM_E_SHAPE;
  if (h->ctx != nullptr && (h->ctx_len == nullptr || h->ctx_idx == nullptr)) return UNIMM_E_ARG;
  if (h->ctx != nullptr && (h->nctx < 1 || h->ldc < 0 || h->ldc > CTX_MAX)) return UNIMM_E_SHAPE;
  out->hist = h->hist; out->hist_len = h->hist_len; out->ctx = h->ctx; out->ctx_len = h->ctx_len; out->ctx_idx = h->ctx_idx;
  out->ldh = h->ldh; out->nctx = h->nctx; out->ldc = h->ldc; out->ngram = h->ngram; out->sep = h->sep;
  out->penalty = h->penalty; out->inv_penalty = h->inv_penalty;
  return UNIMM_OK;
}

}  // namespace

extern "C" int unimm_lm_topk_hist(const float* logits, int32_t rows, int32_t V, int32_t ldl, const int32_t* banned,
                                  int32_t nbanned, const int32_t* flags, int32_t sep, int32_t K, const unimm_lm_history* history,
                                  float* vals, int32_t* ids, float* lse, void* stream) {
  if (logits == nullptr || vals == nullptr || ids == nullptr || (nbanned > 0 && banned == nullptr)) return UNIMM_E_ARG;
  TopkParams p;
  if (const int rc = read_history(history, &p.h)) return rc;
  if (rows < 0 || V < 1 || V > VMAX || ldl < V || K < 1 || K > TOPK_MAX || K > V || nbanned < 0) return UNIMM_E_SHAPE;
  if (rows == 0) return UNIMM_OK;
  p.logits = logits; p.banned = banned; p.flags = flags; p.vals = vals; p.ids = ids; p.lse = lse;
  p.rows = rows; p.V = V; p.ldl = ldl; p.nbanned = nbanned; p.sep = sep; p.K = K;
  hipLaunchKernelGGL(lm_topk_kernel<true>, dim3((unsigned)rows), dim3(NTHREADS), 0, (hipStream_t)stream, p);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

extern "C" int unimm_lm_sample(const float* logits, int32_t rows, int32_t V, int32_t ldl, const int32_t* banned, int32_t nbanned,
                               const int32_t* flags, int32_t sep, float temperature, int32_t top_k, float top_p, uint32_t key,
                               const int32_t* stream_ids, int32_t* token, float* logp, float* logq, float* lse, void* stream) {
  if (logits == nullptr || stream_ids == nullptr || token == nullptr || logp == nullptr || logq == nullptr ||
      (nbanned > 0 && banned == nullptr))
    return UNIMM_E_ARG;
  if (!(temperature > 0.f) || !(temperature < INFINITY) || !(top_p > 0.f && top_p <= 1.f) || top_k < 0) return UNIMM_E_ARG;
  if (rows < 0 || V < 1 || V > VMAX || ldl < V || nbanned < 0) return UNIMM_E_SHAPE;
  if (rows == 0) return UNIMM_OK;
  SampleParams p;
  p.logits = logits; p.banned = banned; p.flags = flags; p.stream = stream_ids;
  p.token = token; p.logp = logp; p.logq = logq; p.lse = lse;
  p.rows = rows; p.V = V; p.ldl = ldl; p.nbanned = nbanned; p.sep = sep; p.top_k = top_k;
  p.temperature = temperature; p.top_p = top_p; p.key = key;
  p.temp_rows = nullptr; p.topk_rows = nullptr; p.topp_rows = nullptr;
  p.h = HistParams{};
  return launch_lm_sample<false, false>(p, (hipStream_t)stream);
}

extern "C" int unimm_lm_sample_rows(const float* logits, int32_t rows, int32_t V, int32_t ldl, const int32_t* banned,
                                    int32_t nbanned, const int32_t* flags, int32_t sep, const float* temperature,
                                    const int32_t* top_k, const float* top_p, uint32_t key, const int32_t* stream_ids,
                                    int32_t* token, float* logp, float* logq, float* lse, void* stream) {
  if (logits == nullptr || stream_ids == nullptr || token == nullptr || logp == nullptr || logq == nullptr ||
      (nbanned > 0 && banned == nullptr) || temperature == nullptr || top_k == nullptr || top_p == nullptr)
    return UNIMM_E_ARG;
  if (rows < 0 || V < 1 || V > VMAX || ldl < V || nbanned < 0) return UNIMM_E_SHAPE;
  if (rows == 0) return UNIMM_OK;
  SampleParams p;
  p.logits = logits; p.banned = banned; p.flags = flags; p.stream = stream_ids;
  p.token = token; p.logp = logp; p.logq = logq; p.lse = lse;
  p.rows = rows; p.V = V; p.ldl = ldl; p.nbanned = nbanned; p.sep = sep; p.top_k = 0;
  p.temperature = 1.f; p.top_p = 1.f; p.key = key;
  p.temp_rows = temperature; p.topk_rows = top_k; p.topp_rows = top_p;
  p.h = HistParams{};
  return launch_lm_sample<true, false>(p, (hipStream_t)stream);
}

extern "C" int unimm_lm_sample_hist(const float* logits, int32_t rows, int32_t V, int32_t ldl, const int32_t* banned,
                                    int32_t nbanned, const int32_t* flags, int32_t sep, const float* temperature,
                                    const int32_t* top_k, const float* top_p, uint32_t key, const int32_t* stream_ids,
                                    const unimm_lm_history* history, int32_t* token, float* logp, float* logq, float* lse,
                                    void* stream) {
  if (logits == nullptr || stream_ids == nullptr || token == nullptr || logp == nullptr || logq == nullptr ||
      (nbanned > 0 && banned == nullptr) || temperature == nullptr || top_k == nullptr || top_p == nullptr)
    return UNIMM_E_ARG;
  SampleParams p;
  if (const int rc = read_history(history, &p.h)) return rc;
  if (rows < 0 || V < 1 || V > VMAX || ldl < V || nbanned < 0) return UNIMM_E_SHAPE;
  if (rows == 0) return UNIMM_OK;
  p.logits = logits; p.banned = banned; p.flags = flags; p.stream = stream_ids;
  p.token = token; p.logp = logp; p.logq = logq; p.lse = lse;
  p.rows = rows; p.V = V; p.ldl = ldl; p.nbanned = nbanned; p.sep = sep; p.top_k = 0;
  p.temperature = 1.f; p.top_p = 1.f; p.key = key;
  p.temp_rows = temperature; p.topk_rows = top_k; p.topp_rows = top_p;
  return launch_lm_sample<true, true>(p, (hipStream_t)stream);
}

extern "C" int unimm_lm_spec_verify(const unimm_lm_spec_verify_args* a, void* stream) {
  if (a == nullptr || a->x == nullptr || a->xd == nullptr || a->draft_token == nullptr || a->stream_ids == nullptr ||
      a->temperature == nullptr || a->top_k == nullptr || a->top_p == nullptr || a->accept == nullptr || a->token == nullptr ||
      a->logp == nullptr || a->logq == nullptr || a->lse == nullptr || (a->nbanned > 0 && a->banned == nullptr))
    return UNIMM_E_ARG;
  if (a->rows < 0 || a->V < 1 || a->V > VMAX || a->ldl < a->V || a->ldd < a->V || a->nbanned < 0) return UNIMM_E_SHAPE;
  if (a->rows == 0) return UNIMM_OK;
  SpecParams p;
  p.x = a->x; p.xd = a->xd; p.draft = a->draft_token; p.banned = a->banned; p.flags = a->flags; p.stream = a->stream_ids;
  p.temp_rows = a->temperature; p.topk_rows = a->top_k; p.topp_rows = a->top_p;
  p.accept = a->accept; p.token = a->token; p.logp = a->logp; p.logq = a->logq; p.lse = a->lse; p.log_ratio = a->log_ratio;
  p.rows = a->rows; p.V = a->V; p.ldl = a->ldl; p.ldd = a->ldd; p.nbanned = a->nbanned; p.sep = a->sep;
  p.key_accept = a->key_accept; p.key_residual = a->key_residual;
  if (p.V <= STAGE_MAX) {
    static bool done = false;
    if (!done) {
      if (hipFuncSetAttribute((const void*)lm_spec_verify_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              STAGE_MAX * (int)sizeof(uint32_t)) != hipSuccess)
        return UNIMM_E_HIP;
      done = true;
    }
    hipLaunchKernelGGL(lm_spec_verify_kernel<true>, dim3((unsigned)p.rows), dim3(NTHREADS), (size_t)p.V * sizeof(uint32_t),
                       (hipStream_t)stream, p);
  } else {
    hipLaunchKernelGGL(lm_spec_verify_kernel<false>, dim3((unsigned)p.rows), dim3(NTHREADS), 0, (hipStream_t)stream, p);
  }
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}
