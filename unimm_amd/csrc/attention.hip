// Fused masked attention cores for the UniMM-UL hot path (gfx950): forward, dQ and dK/dV kernels.
//
// Replaces softmax(Q K^T / sqrt(d) + mask) . V with attention-prob dropout, in the four shapes of
// the reference: text self-attention (T=256, d=64, dense per-sequence mask;
// models/vilbert_dialog.py:390-410), visual self-attention (R=37, d=128, key-padding mask; :519-539)
// and both directions of the co-attention (:681-721).  No score matrix ever reaches HBM.
//
// Structure (one workgroup = one (sequence, head); one wave = one 32-query tile):
//   * K and V of the head are staged once into LDS (<= 256 keys x d fits: 64 KiB at d=64).
//   * S^T = K . Q^T with v_mfma_f32_32x32x16_bf16 ("swapped" product): the query sits on the lane,
//     keys in the 16 accumulator registers, so row max / row sum are register reductions plus one
//     cross-half exchange, and the whole 256-key row stays in registers (exact softmax, no online
//     rescaling needed at T <= 256).
//   * masks are bit-packed (1 bit per (query,key), 8 KiB per sequence instead of 512 KiB int64);
//     masked scores get the reference's additive -10000 (not -inf), so fully masked rows reproduce
//     softmax(raw scores) exactly as models/vilbert_dialog.py:1418 does.
//   * P (bf16) feeds O^T = V^T . P^T directly from the accumulator registers (its key index is the
//     MFMA's reduction index); V^T fragments come from ds_read_b64_tr_b16.
#include <initializer_list>
#include <type_traits>
#include "common.h"

// ---- A/B defaults (tools/build_variant.sh passes -D): 1 = what ships ----------------------------
#ifndef UNIMM_ATTN_TILE_SWZ
#define UNIMM_ATTN_TILE_SWZ 1      // 0 = the unswizzled dS^T / P tile (tile64_swz)
#endif
#ifndef UNIMM_ATTN_FEWQ_FWD
#define UNIMM_ATTN_FEWQ_FWD 1      // 0 = attn_fwd_kernel<128, 8> for the few-query forward shape, as rounds 1-5
#endif
#ifndef UNIMM_ATTN_FEWQ128
#define UNIMM_ATTN_FEWQ128 1       // 0 = the dQ + dK/dV kernel pair for the 37-query directions too
#endif
#ifndef UNIMM_ATTN_FEWK128
#define UNIMM_ATTN_FEWK128 1       // 0 = the kernel pair for the text-attends-regions direction
#endif

namespace {

// ---- LDS layouts --------------------------------------------------------------------------------
// A kernel that carves `extern __shared__ char smem[]` has ONE layout type next to it (…Lds): the byte offset of every region and
// the total `bytes`.  The kernel forms its pointers as smem + L::region and its launch passes L::bytes, so a region cannot be
// added on one side only (an LDS access past the allocation does not fault here: it is dropped or reads zero).  Every layout
// asserts that it fits a CU and that the regions accessed 16 bytes at a time start on a multiple of 16.
constexpr int LDS_CU_BYTES = 160 * 1024;
constexpr bool lds_aligned16(std::initializer_list<int> offsets) {
  for (int o : offsets) if (o % 16 != 0) return false;
  return true;
}

struct AttnParams {
  const bf16_t* q; const bf16_t* k; const bf16_t* v;
  bf16_t* o; float* lse;
  const uint32_t* mask;  // [B][mask rows][nw] words, bit j of word t = key 32t+j may be attended
  // variable-length ("unpadded") mode: sequence b owns rows [off[b], off[b]+len[b]) of the packed q / kv
  // matrices; NULL = fixed layout (rows b*T .. b*T+T-1).  Tq/Tk stay the PADDED lengths: they index the
  // mask, lse and dropout counters, so a packed run reproduces the padded run bit for bit on valid rows.
  const int* q_off; const int* q_len; const int* k_off; const int* k_len;
  // forward only: a SHARED key/value segment (rows [ks_off[b], ks_off[b] + ks_len[b]) of the same k / v matrices) spliced into
  // sequence b's keys after its first ks_ins private rows: key position j is private row j (j < ks_ins), shared row j - ks_ins,
  // or private row j - ks_len[b].  The sequence then has k_len[b] + ks_len[b] keys; mask words index key POSITIONS.  What the
  // candidates of one dialog round use to attend the round's context rows, computed once (unimm_amd/scoring.py).
  const int* ks_off; const int* ks_len; int ks_ins;
  // or NULL: a permutation of the sequences; workgroups take their (sequence, head) items in THIS order.  With variable lengths
  // the longest sequences first: the dispatcher hands items to free CU slots in grid order, so the launch's tail is then made of
  // the shortest items instead of whatever the batch order put last (the step's plan writes it: unimm_plan_build).
  const int* order;
  int B, H, Tq, Tk, ldq, ldk, ldv, ldo;
  int mask_q_stride, mask_b_stride;  // in words; q stride 0 = one row per sequence (key padding)
  int parts;                          // workgroups per (sequence, head): each owns a contiguous run of 32-row tiles
  float scale;
  DropoutArg drop;
};

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

// ---- LDS images -------------------------------------------------------------------------------
// Rows of D bf16 (2D bytes = D/8 chunks of 16 B), 16-B chunk index XOR-swizzled per row with ONE
// function that keeps both kinds of read conflict-free: ds_read_b128 row fragments (a 16-lane group
// reads 16 rows at one chunk) and ds_read_b64_tr_b16 transposed fragments (a 32-lane half reads
// 4 rows x 64 B).  D=128 is the guide's image (b); D=64 is its 128-B-row analogue.
template <int D> __device__ __forceinline__ int swz(int row) {
  if constexpr (D == 64) { const int t = row >> 1; return (t & 7) ^ ((t & 1) << 2); }
  else return ((row & 3) << 2) | ((row >> 2) & 3);
}

// Cooperative stage of `nrows_pad` (multiple of 32) rows of one head; rows >= nrows are zero-filled.
// LDS-DMA: one wave-instruction lands 1 KiB lane-linearly (4 rows of D=128, 8 rows of D=64), so lane l
// of a group supplies the 16-byte chunk that belongs at physical position l of those rows -- the chunk
// swizzle is applied on the SOURCE address.  Every load of both images is in flight before the first
// one returns (the register-staged version paid a load->ds_write round trip per 16 bytes per thread).
// The caller waits vmcnt(0) before its barrier.
template <int D>
__device__ __forceinline__ void stage_head(const bf16_t* __restrict__ g, int ld, int nrows, int nrows_pad,
                                           char* img, int tid, int nthreads) {
  constexpr int CPR = D / 8;        // 16-byte chunks per row
  constexpr int RPI = 64 / CPR;     // rows per wave-instruction
  const int wave = tid >> 6, lane = tid & 63, nwaves = nthreads >> 6;
  const int rl = lane / CPR, pc = lane % CPR;
  for (int grp = wave; grp < nrows_pad / RPI; grp += nwaves) {
    const int row = grp * RPI + rl;
    if (row < nrows) {
      const bf16_t* src = g + (size_t)row * ld + ((pc ^ swz<D>(row)) << 3);
      __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(img + grp * 1024), 16, 0, 0);
    } else {
      *reinterpret_cast<u32x4*>(img + grp * 1024 + lane * 16) = u32x4{0u, 0u, 0u, 0u};
    }
  }
}
// The same with the rows of a spliced key sequence (AttnParams.ks_*): base = first element of the head in row 0 of the matrix.
template <int D>
__device__ __forceinline__ void stage_head_seg(const bf16_t* __restrict__ base, int ld, size_t kbase, size_t sbase, int ins, int slen,
                                               int nrows, int nrows_pad, char* img, int tid, int nthreads) {
  constexpr int CPR = D / 8, RPI = 64 / CPR;
  const int wave = tid >> 6, lane = tid & 63, nwaves = nthreads >> 6;
  const int rl = lane / CPR, pc = lane % CPR;
  for (int grp = wave; grp < nrows_pad / RPI; grp += nwaves) {
    const int row = grp * RPI + rl;
    if (row < nrows) {
      const size_t grow = row < ins ? kbase + row : (row < ins + slen ? sbase + (row - ins) : kbase + (row - slen));
      const bf16_t* src = base + grow * ld + ((pc ^ swz<D>(row)) << 3);
      __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(img + grp * 1024), 16, 0, 0);
    } else {
      *reinterpret_cast<u32x4*>(img + grp * 1024 + lane * 16) = u32x4{0u, 0u, 0u, 0u};
    }
  }
}
__device__ __forceinline__ void stage_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

template <int D> __device__ __forceinline__ bf16x8 read_row_frag(const char* img, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(img + row * (2 * D) + ((chunk ^ swz<D>(row)) << 4));
}

// transposed 32x32x16 operand (permuted reduction order, cdna guide 3 "accumulator tile as operand"):
// element j of lane (r = lane&31, h = lane>>5) = img[rowbase + 8*(j>>2) + 4h + (j&3)][col0 + r]
template <int D>
__device__ __forceinline__ bf16x8 read_tr_frag(const char* img, int rowbase, int col0, int lane) {
  const int h = lane >> 5, i = lane & 15, qq = i >> 2, pp = i & 3;
  const int col = col0 + 16 * ((lane >> 4) & 1) + 4 * pp;
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  s16x4 part[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int row = rowbase + 8 * jj + 4 * h + qq;
    const int pch = (col >> 3) ^ swz<D>(row);
    part[jj] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)LDS_PTR(img + row * (2 * D) + pch * 16 + (col & 7) * 2));
  }
  s16x8 v = {part[0][0], part[0][1], part[0][2], part[0][3], part[1][0], part[1][1], part[1][2], part[1][3]};
  return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ bf16x8 pack8(const float* p) {
  typedef __attribute__((ext_vector_type(4))) unsigned int u4;
  u4 w = {pack2bf(p[0], p[1]), pack2bf(p[2], p[3]), pack2bf(p[4], p[5]), pack2bf(p[6], p[7])};
  return __builtin_bit_cast(bf16x8, w);
}

__device__ __forceinline__ int key_of_reg(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// Row store of a transposed 32x32 accumulator set (lane = row, registers = D values): the MFMA layout leaves a lane 4
// consecutive values of every 8 -- its partner lane ^ 32 (same row) holds the other 4 -- so the direct form is one 8-byte piece
// per lane and group of 8: 2 D / 8 store instructions per row tensor, and the kernels' result stores are store-ISSUE bound
// (with them compiled out the text backward drops 275 -> 235 us, the 37-region sides 226 -> 186 / 245 -> 185: twice what the
// bytes need).  Partner lanes trade pieces with v_permlane32_swap: a lane then owns all 8 values of every second group and
// writes them as ONE 16-byte store -- half the instructions.  Executed by all lanes (the swap), stored where `ok`.
template <int D>
__device__ __forceinline__ void store_acc_row(bf16_t* __restrict__ g, const f32x16 (&a)[D / 32], float s, int h, bool ok) {
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int qp = 0; qp < 2; ++qp) {
      const uint32_t a0 = pack2bf(a[dt][8 * qp] * s, a[dt][8 * qp + 1] * s), a1 = pack2bf(a[dt][8 * qp + 2] * s, a[dt][8 * qp + 3] * s);
      const uint32_t b0 = pack2bf(a[dt][8 * qp + 4] * s, a[dt][8 * qp + 5] * s), b1 = pack2bf(a[dt][8 * qp + 6] * s, a[dt][8 * qp + 7] * s);
      // swap(x, y): x's lanes 32..63 <-> y's lanes 0..31.  h = 0 lanes end with (own group 2 qp | partner's group 2 qp),
      // h = 1 lanes with (partner's group 2 qp + 1 | own group 2 qp + 1): 8 consecutive values either way
      const auto w0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
      const auto w1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
      if (ok) *reinterpret_cast<u32x4*>(g + 32 * dt + 16 * qp + 8 * h) = u32x4{w0[0], w1[0], w0[1], w1[1]};
    }
}

// LDS of attn_fwd_kernel and attn_bwd_dq_kernel: the K and V images of the (sequence, head)
template <int D, int NKT>
struct KvImagesLds {
  static constexpr int KPAD = NKT * 32;
  static constexpr int kimg = 0;                          // [KPAD keys][D] bf16, chunk-swizzled (swz)
  static constexpr int vimg = kimg + KPAD * 2 * D;        // the same of V
  static constexpr int bytes = vimg + KPAD * 2 * D;
  static_assert(bytes <= LDS_CU_BYTES);
  static_assert(lds_aligned16({kimg, vimg}));
};

template <int D, int NKT>
__global__ __launch_bounds__(512, 2) void attn_fwd_kernel(AttnParams p) {
  drop_resolve(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using L = KvImagesLds<D, NKT>;
  constexpr int KPAD = NKT * 32;
  char *kimg = smem + L::kimg, *vimg = smem + L::vimg;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int item = blockIdx.x / p.parts, part = blockIdx.x % p.parts;
  const int b = p.order != nullptr ? p.order[item / p.H] : item / p.H, head = item % p.H;
  const int nwv = blockDim.x >> 6;                     // waves of this workgroup: wave w owns query tiles w, w + nwv, ...
  const int r = lane & 31, h = lane >> 5;

  const int Ts_b = p.ks_len ? p.ks_len[b] : 0;                                  // spliced shared keys (AttnParams.ks_*)
  int Tk_b = (p.k_len ? p.k_len[b] : p.Tk) + Ts_b;
  Tk_b = Tk_b < KPAD ? Tk_b : KPAD;                                             // (the images hold KPAD rows; the host checks the sum)
  const int Tq_b = p.q_len ? p.q_len[b] : p.Tq;
  if (part * (int)(blockDim.x >> 6) * 32 >= Tq_b) return;   // whole workgroup is padding: nothing staged
  const size_t qbase = p.q_off ? (size_t)p.q_off[b] : (size_t)b * p.Tq;
  const size_t kbase = p.k_off ? (size_t)p.k_off[b] : (size_t)b * p.Tk;
  const size_t sbase = p.ks_off ? (size_t)p.ks_off[b] : 0;
  const int kpad_b = ((Tk_b + 31) & ~31) < KPAD ? ((Tk_b + 31) & ~31) : KPAD;   // key tiles past it are skipped
  stage_head_seg<D>(p.k + head * D, p.ldk, kbase, sbase, p.ks_ins, Ts_b, Tk_b, kpad_b, kimg, tid, blockDim.x);
  stage_head_seg<D>(p.v + head * D, p.ldv, kbase, sbase, p.ks_ins, Ts_b, Tk_b, kpad_b, vimg, tid, blockDim.x);

  // Q fragments straight from HBM (each element is used once per key tile, by this wave only) and the mask words
  // of the query row; the first tile's are requested before the staging barrier
  int wt = part * nwv + wave;
  int q0, qrow;
  bool qvalid;
  bf16x8 qf[D / 16];
  uint32_t mw[NKT];
#define UNIMM_LOAD_QTILE()                                                                                    \
  {                                                                                                          \
    q0 = wt * 32;                                                                                            \
    qrow = q0 + r;                                                                                           \
    qvalid = qrow < Tq_b;                                                                                    \
    if (!qvalid) qrow = Tq_b - 1;                                                                            \
    const bf16_t* qg_ = p.q + (qbase + qrow) * p.ldq + head * D;                                             \
    _Pragma("unroll") for (int ks = 0; ks < D / 16; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qg_ + 16 * ks + 8 * h); \
    const uint32_t* mp_ = p.mask + (size_t)b * p.mask_b_stride + (size_t)qrow * p.mask_q_stride;            \
    _Pragma("unroll") for (int t = 0; t < NKT; ++t) mw[t] = 32 * t < p.Tk ? mp_[t] : 0u;   /* a row has ceil(Tk / 32) words */ \
  }
  UNIMM_LOAD_QTILE()
  stage_wait();
  __syncthreads();
  // A wave walks its query tiles one after the other.  With 8 tiles on 4 waves, two workgroups fit a CU and every
  // resident wave has work: with one wave per tile, the tiles past a sequence's length were waves that exited at
  // once and left the CU (one 8-wave workgroup at these register counts) half empty for the average dialog.
  constexpr bool WALK = D == 64;     // D = 128 instances are at their register limit: one tile per wave there
  for (bool first = true; wt * 32 < Tq_b && (WALK || first); first = false, wt += nwv * p.parts) {
    if (WALK && !first) UNIMM_LOAD_QTILE()

  // ---- S^T = K . Q^T, all (non-padding) key tiles kept in registers
  f32x16 s[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    f32x16 acc = {};
    if (32 * t < Tk_b) {
#pragma unroll
      for (int ks = 0; ks < D / 16; ++ks) {
        const bf16x8 kf = read_row_frag<D>(kimg, 32 * t + r, 2 * ks + h);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], acc, 0, 0, 0);
      }
    }
    s[t] = acc;
  }

  // ---- mask + softmax over the lane's 16*NKT keys and its partner's (lane ^ 32), in the log2 domain:
  // v = s * (scale * log2 e) + (masked ? -10000 * log2 e : 0) is ONE fma per score -- the additive mask (reference
  // :1418) is the sign-extended inverted mask bit ANDed with the constant's bit pattern (v_bfe_i32 + v_and) instead of
  // shift / and / compare / select / add -- and the "key exists" test runs only on the sequence's last, partial tile.
  const float c1 = p.scale * LOG2E;
  constexpr float MOFF = -10000.0f * LOG2E;
  // (opaque copy: the 128 "key exists" compares are invariant over this wave's query tiles, and hoisted out of the walk
  // the compiler parked their lane masks in SGPRs, spilled them to VGPR lanes and read two lanes back per score)
  int tk_here = Tk_b;
  asm volatile("" : "+v"(tk_here));
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    if (32 * t >= Tk_b) continue;                          // (wave-uniform) tile holds padding keys only
    const uint32_t wn = ~(mw[t] >> (4 * h));               // bit kk set = key kk (+ 4h folded in) is masked
    auto scores = [&](auto partial) {
#pragma unroll
      for (int e = 0; e < 16; e += 2) {                    // registers e, e + 1 = keys kk, kk + 1: one packed fma for the pair
        const int kk = (e & 3) + 8 * (e >> 2);
        f32x2v madd;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const uint32_t mb = (uint32_t)__builtin_amdgcn_sbfe((int)wn, kk + u, 1) & __builtin_bit_cast(uint32_t, MOFF);
          madd[u] = __uint_as_float(mb);
          if constexpr (decltype(partial)::value)           // padded keys do not exist
            madd[u] = (32 * t + kk + u + 4 * h) < tk_here ? madd[u] : -INFINITY;
        }
        const f32x2v v = f32x2v{s[t][e], s[t][e + 1]} * c1 + madd;
        s[t][e] = v.x; s[t][e + 1] = v.y;
        mx = fmaxf(mx, fmaxf(v.x, v.y));
      }
    };
    if (32 * (t + 1) > Tk_b) scores(std::true_type{}); else scores(std::false_type{});
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  f32x2v sum2 = {0.f, 0.f};
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    if (32 * t >= Tk_b) continue;
#pragma unroll
    for (int e = 0; e < 16; e += 2) {
      const f32x2v a = f32x2v{s[t][e], s[t][e + 1]} - mx;
      const float p0 = __builtin_amdgcn_exp2f(a.x), p1 = __builtin_amdgcn_exp2f(a.y);
      s[t][e] = p0; s[t][e + 1] = p1;
      sum2 += f32x2v{p0, p1};
    }
  }
  float sum = sum2.x + sum2.y;
  sum += __shfl_xor(sum, 32, 64);
  // the dropout scale 1 / (1 - p) rides on the normalisation: the keep test below is a plain select
  const float inv = (p.drop.thr != 0u ? p.drop.scale : 1.0f) / sum;

  if (p.drop.thr != 0u) {
    // one hash per two neighbouring keys (registers e, e+1 with e even hold keys k, k+1 with k even)
    // linear stage of the hash: per-lane constant (query row, lane half) + a compile-time multiple of M1 per (tile, register pair)
    const uint32_t wl = drop_lin(p.drop, drop_wbase(((uint32_t)b * p.H + head) * p.Tq + (uint32_t)qrow, (uint32_t)p.Tk, 0u) + 2u * (uint32_t)h);
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      if (32 * t >= Tk_b) continue;
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        const uint32_t w = drop_fin(p.drop, wl + (uint32_t)((32 * t + key_of_reg(e, 0)) >> 1) * DROP_M1);
        s[t][e] = drop_keep(p.drop, w, 0u) ? s[t][e] : 0.0f;
        s[t][e + 1] = drop_keep(p.drop, w, 1u) ? s[t][e + 1] : 0.0f;
      }
    }
  }

  // ---- O^T = V^T . P^T
  f32x16 o[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) o[dt] = f32x16{};
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    if (32 * t >= Tk_b) continue;
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      float pv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pv[j] = s[t][8 * ss + j];
      const bf16x8 pf = pack8(pv);
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) {
        const bf16x8 vf = read_tr_frag<D>(vimg, 32 * t + 16 * ss, 32 * dt, lane);
        o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[dt], 0, 0, 0);
      }
    }
  }

  store_acc_row<D>(p.o + (qbase + (qvalid ? qrow : 0)) * p.ldo + head * D, o, inv, h, qvalid);
  if (qvalid) {
    if (p.lse != nullptr && h == 0) p.lse[((size_t)b * p.H + head) * p.Tq + qrow] = (mx + __log2f(sum)) * LN2;
  }
  }   // query tiles of this wave
#undef UNIMM_LOAD_QTILE
}


// ------------------------------------------------------------------------------------------------
// backward, part 1: dQ (query on the lane, same walk as the forward) + delta = rowsum(dO o O)
//   P = exp(S' - lse);  dP = dO . V^T (dropout mask re-generated);  dS = scale * P o (dP - delta)
//   dQ^T += K^T . dS^T    (K^T fragments: transposed reads of the same K image)
// ------------------------------------------------------------------------------------------------
struct AttnBwdParams {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; const bf16_t* o; const bf16_t* dout;
  const float* lse; float* delta;
  bf16_t* dq; bf16_t* dk; bf16_t* dv;
  const uint32_t* mask;
  const int* q_off; const int* q_len; const int* k_off; const int* k_len;
  const int* order;      // as AttnParams.order
  int B, H, Tq, Tk, ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
  int mask_q_stride, mask_b_stride;
  int parts;
  float scale;
  DropoutArg drop;
};

template <int D, int NKT>
__global__ __launch_bounds__(512, 2) void attn_bwd_dq_kernel(AttnBwdParams p) {
  drop_resolve(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using L = KvImagesLds<D, NKT>;
  constexpr int KPAD = NKT * 32;
  char *kimg = smem + L::kimg, *vimg = smem + L::vimg;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int item = blockIdx.x / p.parts, part = blockIdx.x % p.parts;
  const int b = p.order != nullptr ? p.order[item / p.H] : item / p.H, head = item % p.H;
  const int wt = part * (blockDim.x >> 6) + wave;
  const int r = lane & 31, h = lane >> 5;

  const int Tq_b = p.q_len ? p.q_len[b] : p.Tq, Tk_b = p.k_len ? p.k_len[b] : p.Tk;
  if (part * (int)(blockDim.x >> 6) * 32 >= Tq_b) return;
  const size_t qbase = p.q_off ? (size_t)p.q_off[b] : (size_t)b * p.Tq;
  const size_t kbase = p.k_off ? (size_t)p.k_off[b] : (size_t)b * p.Tk;
  const int kpad_b = ((Tk_b + 31) & ~31) < KPAD ? ((Tk_b + 31) & ~31) : KPAD;
  stage_head<D>(p.k + kbase * p.ldk + head * D, p.ldk, Tk_b, kpad_b, kimg, tid, blockDim.x);
  stage_head<D>(p.v + kbase * p.ldv + head * D, p.ldv, Tk_b, kpad_b, vimg, tid, blockDim.x);

  int qrow = wt * 32 + r;
  const bool qvalid = qrow < Tq_b;
  if (!qvalid) qrow = Tq_b - 1;
  const size_t grow = qbase + qrow;
  const bf16_t* qg = p.q + grow * p.ldq + head * D;
  const bf16_t* dog = p.dout + grow * p.lddo + head * D;
  const bf16_t* og = p.o + grow * p.ldo + head * D;
  bf16x8 qf[D / 16], dof[D / 16];
  float delta = 0.f;
#pragma unroll
  for (int ks = 0; ks < D / 16; ++ks) {
    qf[ks] = *reinterpret_cast<const bf16x8*>(qg + 16 * ks + 8 * h);
    dof[ks] = *reinterpret_cast<const bf16x8*>(dog + 16 * ks + 8 * h);
    const bf16x8 of = *reinterpret_cast<const bf16x8*>(og + 16 * ks + 8 * h);
#pragma unroll
    for (int j = 0; j < 8; ++j) delta += (float)dof[ks][j] * (float)of[j];
  }
  delta += __shfl_xor(delta, 32, 64);
  const size_t stat = ((size_t)b * p.H + head) * p.Tq + qrow;
  const float lse_l = p.lse[stat] * LOG2E;
  if (qvalid && h == 0) p.delta[stat] = delta;

  uint32_t mw[NKT];
  {
    const uint32_t* mp = p.mask + (size_t)b * p.mask_b_stride + (size_t)qrow * p.mask_q_stride;
#pragma unroll
    for (int t = 0; t < NKT; ++t) mw[t] = 32 * t < p.Tk ? mp[t] : 0u;   // a row has ceil(Tk / 32) words: tiles past them are skipped
  }
  stage_wait();
  __syncthreads();
  if (wt * 32 >= Tq_b) return;

  f32x16 dq[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) dq[dt] = f32x16{};
  const uint32_t dwl = drop_lin(p.drop, drop_wbase(((uint32_t)b * p.H + head) * p.Tq + (uint32_t)qrow, (uint32_t)p.Tk, 0u) + 2u * (uint32_t)h);

  // Per score (same log2-domain form as the forward): arg = s * c1 + (masked ? -10000 log2 e : 0) - lse log2 e is one
  // fma, because -lse / scale is what the S accumulator STARTS from; the dropout select carries 1 / (1 - p) and feeds an
  // fma with -delta; the softmax scale is applied once to dQ at the end instead of to every dS.
  const float c1 = p.scale * LOG2E;
  constexpr float MOFF = -10000.0f * LOG2E;
  const float s0 = -lse_l / c1;
  const bool dropping = p.drop.thr != 0u;
  const uint32_t thr16 = dropping ? (p.drop.thr >> 16) : 0u;
  const float dsc = dropping ? p.drop.scale : 1.0f;
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    if (32 * t >= Tk_b) break;
    f32x16 sacc, dpacc = {};
#pragma unroll
    for (int e = 0; e < 16; ++e) sacc[e] = s0;
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      const bf16x8 kf = read_row_frag<D>(kimg, 32 * t + r, 2 * ks + h);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], sacc, 0, 0, 0);
      const bf16x8 vf = read_row_frag<D>(vimg, 32 * t + r, 2 * ks + h);
      dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dof[ks], dpacc, 0, 0, 0);
    }
    const uint32_t wn = ~(mw[t] >> (4 * h));
    float ds[16];
    uint32_t dw[8];   // dropout words: one hash per two neighbouring keys
    if (dropping) {
#pragma unroll
      for (int e2 = 0; e2 < 8; ++e2) dw[e2] = drop_fin(p.drop, dwl + (uint32_t)((32 * t + key_of_reg(2 * e2, 0)) >> 1) * DROP_M1);
    } else {
#pragma unroll
      for (int e2 = 0; e2 < 8; ++e2) dw[e2] = 0u;          // with thr16 = 0 every field "keeps", at scale 1
    }
    // Straight-line per score (no per-element branch: without dropout the keep test is simply always true), one
    // instance with the "key exists" select on every tile: the unrolled tile loop is 8 copies of this already, and a
    // second, select-free copy per tile made the D = 128 instances slower (code size and registers).
#pragma unroll
    for (int e = 0; e < 16; e += 2) {                      // registers e, e + 1 = keys kk, kk + 1: packed fp32 math on the pair
      const int kk = (e & 3) + 8 * (e >> 2);
      f32x2v madd, tkv;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const uint32_t mb = (uint32_t)__builtin_amdgcn_sbfe((int)wn, kk + u, 1) & __builtin_bit_cast(uint32_t, MOFF);
        madd[u] = (32 * t + kk + u + 4 * h) < Tk_b ? __uint_as_float(mb) : -INFINITY;   // padded keys: P = 0
        const uint32_t field = u ? (dw[e >> 1] >> 16) : (dw[e >> 1] & 0xffffu);
        tkv[u] = field >= thr16 ? dsc : 0.0f;
      }
      const f32x2v arg = f32x2v{sacc[e], sacc[e + 1]} * c1 + madd;
      f32x2v pe;
      pe.x = __builtin_amdgcn_exp2f(arg.x); pe.y = __builtin_amdgcn_exp2f(arg.y);
      const f32x2v dsv = pe * (f32x2v{dpacc[e], dpacc[e + 1]} * tkv - delta);
      ds[e] = dsv.x; ds[e + 1] = dsv.y;
    }
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      const bf16x8 dsf = pack8(ds + 8 * ss);
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) {
        const bf16x8 ktf = read_tr_frag<D>(kimg, 32 * t + 16 * ss, 32 * dt, lane);
        dq[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf, dsf, dq[dt], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) dq[dt][e] *= p.scale;

  store_acc_row<D>(p.dq + (qvalid ? grow : 0) * p.lddq + head * D, dq, 1.0f, h, qvalid);
}

// Keys past the sequence's end do not exist, whatever the mask bits say.  The key-on-the-lane forms compute their lanes anyway (from
// the last key's row), and a set bit would give such a lane P = 2^(s - lse): +inf on a fully masked query row (lse ~ -10000), which
// the zero K^T rows of dQ turn into NaN (0 * inf).  Their inverted words therefore mark those keys masked: P stays finite there.
__device__ __forceinline__ uint32_t pad_key_bits(int Tk_b, int kt) {
  const int n = Tk_b - 32 * kt;                                 // keys of tile kt that exist (>= 1 for the tiles that are staged)
  return n >= 32 ? 0u : ~0u << n;
}

// ------------------------------------------------------------------------------------------------
// backward, part 2: dK, dV (key on the lane; one wave = one 32-key tile, walks all query tiles)
//   S = Q . K^T and dP = dO . V^T land as [query regs][key lane]; P / dS feed
//   dV^T += dO^T . P_drop  and  dK^T += Q^T . dS  straight from the accumulators, with the
//   transposed operands read from the Q / dO images.  No atomics, no cross-wave reduction.
// ------------------------------------------------------------------------------------------------
// MAXT = 256: the variant for <= 2 key tiles (37 region keys) -- 2 compute waves + 2 staging helpers, one wave per
// SIMD and a 512-register budget.  Only launch_bwd_dkv<128, 8> names it, for Tq > 64 and Tk <= 64 -- the shape unimm_attn_bwd
// hands to attn_bwd_fewk128_kernel first, so attn_bwd_dkv_kernel<128, 8, 256> (312 registers, no spills) is reached only by a
// UNIMM_ATTN_FEWK128 = 0 build, and <128, 2, 256> is never instantiated.  What a launch reaches at D = 128 are the MAXT = 512 instances,
// two waves per SIMD, and both spill: <128, 2, 512> (Tq, Tk <= 64: the 37 x 37 image self-attention) is 256 registers with 27 spilled,
// 112 bytes of scratch per lane; <128, 8, 512> (Tq, Tk > 64) 256 with 16 spilled, 68 bytes (tests/test_kernel_resources_cpu.py).
// LDS of this kernel -- and what BwdFusedLds and BwdFewq128Lds begin with: their kernels stage an item's queries the same way
template <int D, int NQT>
struct BwdDkvLds {
  static constexpr int QPAD = NQT * 32;
  static constexpr int qimg = 0;                                    // [QPAD queries][D] bf16, chunk-swizzled (swz)
  static constexpr int doimg = qimg + QPAD * 2 * D;                 // the same of dO
  static constexpr int lse_s = doimg + QPAD * 2 * D;                // [QPAD] fp32: -lse log2 e
  static constexpr int del_s = lse_s + QPAD * (int)sizeof(float);   // [QPAD] fp32: delta
  static constexpr int mw_s = del_s + QPAD * (int)sizeof(float);    // [8 key tiles (waves)][QPAD] inverted mask words
  static constexpr int bytes = mw_s + 8 * QPAD * (int)sizeof(uint32_t);
  static_assert(bytes <= LDS_CU_BYTES);
  static_assert(lds_aligned16({qimg, doimg, lse_s, del_s, mw_s}));
};

template <int D, int NQT, int MAXT = 512>
__global__ __launch_bounds__(MAXT, MAXT == 256 ? 1 : 2) void attn_bwd_dkv_kernel(AttnBwdParams p) {
  drop_resolve(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using L = BwdDkvLds<D, NQT>;
  constexpr int QPAD = NQT * 32;
  char *qimg = smem + L::qimg, *doimg = smem + L::doimg;
  float *lse_s = reinterpret_cast<float*>(smem + L::lse_s), *del_s = reinterpret_cast<float*>(smem + L::del_s);
  uint32_t* mw_s = reinterpret_cast<uint32_t*>(smem + L::mw_s);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int item = blockIdx.x / p.parts, part = blockIdx.x % p.parts;
  const int b = p.order != nullptr ? p.order[item / p.H] : item / p.H, head = item % p.H;
  const int wt = part * (blockDim.x >> 6) + wave;      // this wave's 32-key tile
  const int r = lane & 31, h = lane >> 5;

  const int Tq_b = p.q_len ? p.q_len[b] : p.Tq, Tk_b = p.k_len ? p.k_len[b] : p.Tk;
  if (part * (int)(blockDim.x >> 6) * 32 >= Tk_b) return;
  const size_t qbase = p.q_off ? (size_t)p.q_off[b] : (size_t)b * p.Tq;
  const size_t kbase = p.k_off ? (size_t)p.k_off[b] : (size_t)b * p.Tk;
  const int qpad_b = ((Tq_b + 31) & ~31) < QPAD ? ((Tq_b + 31) & ~31) : QPAD;
  stage_head<D>(p.q + qbase * p.ldq + head * D, p.ldq, Tq_b, qpad_b, qimg, tid, blockDim.x);
  stage_head<D>(p.dout + qbase * p.lddo + head * D, p.lddo, Tq_b, qpad_b, doimg, tid, blockDim.x);
  for (int i = tid; i < qpad_b; i += blockDim.x) {
    const size_t stat = ((size_t)b * p.H + head) * p.Tq + i;
    lse_s[i] = i < Tq_b ? -p.lse[stat] * LOG2E : -INFINITY;   // NEGATED; -inf => P = 0 for padded queries
    del_s[i] = i < Tq_b ? p.delta[stat] : 0.f;
  }
  {
    const int nkt_b = (Tk_b + 31) >> 5;
    const uint32_t* mb = p.mask + (size_t)b * p.mask_b_stride;
    for (int i = tid; i < nkt_b * qpad_b; i += blockDim.x) {
      const int kt = i / qpad_b, qi = i - kt * qpad_b;
      const int qc = qi < Tq_b ? qi : Tq_b - 1;
      mw_s[kt * QPAD + qi] = ~mb[(size_t)qc * p.mask_q_stride + kt] | pad_key_bits(Tk_b, kt);   // INVERTED: bit set = masked
    }
  }

  int krow = wt * 32 + r;
  const bool kvalid = krow < Tk_b;
  if (!kvalid) krow = Tk_b - 1;
  const size_t grow = kbase + krow;
  const bf16_t* kg = p.k + grow * p.ldk + head * D;
  const bf16_t* vg = p.v + grow * p.ldv + head * D;
  bf16x8 kf[D / 16], vf[D / 16];
#pragma unroll
  for (int ks = 0; ks < D / 16; ++ks) {
    kf[ks] = *reinterpret_cast<const bf16x8*>(kg + 16 * ks + 8 * h);
    vf[ks] = *reinterpret_cast<const bf16x8*>(vg + 16 * ks + 8 * h);
  }
  stage_wait();
  __syncthreads();
  if (wt * 32 >= Tk_b) return;

  f32x16 dk[D / 32], dv[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) { dk[dt] = f32x16{}; dv[dt] = f32x16{}; }
  const uint32_t* mrow = mw_s + wt * QPAD;
  const uint32_t hbase = ((uint32_t)b * p.H + head) * (uint32_t)p.Tq;
  const uint32_t halfw = ((uint32_t)p.Tk + 1u) >> 1, halfm = halfw * DROP_M1;      // D = 64 dropout words (see below)
  const uint32_t dlane = drop_lin(p.drop, (4u * (uint32_t)h + ((uint32_t)r & 1u)) * halfw + ((uint32_t)(wt * 32 + r) >> 1));
  const float c1 = p.scale * LOG2E;
  constexpr float MOFF = -10000.0f * LOG2E;
  const bool dropping = p.drop.thr != 0u;
  const uint32_t thr16 = dropping ? (p.drop.thr >> 16) : 0u;
  const float dsc = dropping ? p.drop.scale : 1.0f;

#pragma unroll 1
  for (int qt = 0; qt < NQT; ++qt) {
    if (32 * qt >= Tq_b) break;
    f32x16 sacc = {}, dpacc = {};
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      const bf16x8 qf = read_row_frag<D>(qimg, 32 * qt + r, 2 * ks + h);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kf[ks], sacc, 0, 0, 0);
      const bf16x8 df = read_row_frag<D>(doimg, 32 * qt + r, 2 * ks + h);
      dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, vf[ks], dpacc, 0, 0, 0);
    }
    float pd[16], ds[16];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int qb = 32 * qt + 8 * g4 + 4 * h;   // 4 consecutive queries for registers 4*g4 .. 4*g4+3
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_s + qb);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(del_s + qb);
      const u32x4 w4 = *reinterpret_cast<const u32x4*>(mrow + qb);
      // dropout words: keys k and k^1 (lanes r and r^1) share the hash word of a query row, so each lane of the
      // pair hashes two of the four queries and takes the other two from its neighbour (DPP quad_perm [1,0,3,2])
      uint32_t dwv[4] = {0u, 0u, 0u, 0u};               // without dropout: thr16 = 0, every field "keeps" at scale 1
      uint32_t odd;
      if constexpr (D == 64) {
        odd = (uint32_t)r & 1u;
        if (dropping) {
          // word index (hbase + qb + par [+ 2]) * half + kw, qb = 32 qt + 8 g4 + 4 h: the lane's part of the hash's linear
          // stage (h, par, kw) is loop-invariant, the rest is wave-uniform (scalar multiply)
          const uint32_t par = (uint32_t)r & 1u;
          const uint32_t ua = (hbase + (uint32_t)(32 * qt + 8 * g4)) * halfm;
          const uint32_t wa = drop_fin(p.drop, dlane + ua);
          const uint32_t wb = drop_fin(p.drop, dlane + ua + 2u * halfm);
          const uint32_t oa = (uint32_t)__builtin_amdgcn_mov_dpp((int)wa, 0xB1, 0xF, 0xF, true);
          const uint32_t ob = (uint32_t)__builtin_amdgcn_mov_dpp((int)wb, 0xB1, 0xF, 0xF, true);
          dwv[0] = par ? oa : wa; dwv[1] = par ? wa : oa; dwv[2] = par ? ob : wb; dwv[3] = par ? wb : ob;
        }
      } else {      // D = 128: at its register limit -- one hash per element, inside the loop below, unconditionally
        odd = (uint32_t)krow & 1u;
      }
      // log2-domain score: one fma on top of (-lse log2 e) + (masked ? -10000 log2 e : 0); lanes past the last key need
      // no select -- a key is a lane here, nothing of an invalid lane reaches a valid one and its dK / dV are not stored.
      // Straight-line, two elements at a time (packed fp32 add / fma / mul); the dropout select always runs (dwv above).
      const uint32_t fsh = odd << 4;                       // this lane's 16-bit field of a dropout word
#pragma unroll
      for (int i = 0; i < 4; i += 2) {
        const int e = 4 * g4 + i;
        f32x2v madd, tk;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const uint32_t mb = (uint32_t)__builtin_amdgcn_sbfe((int)w4[i + u], (uint32_t)r, 1) & __builtin_bit_cast(uint32_t, MOFF);
          madd[u] = __uint_as_float(mb);
          uint32_t dwe = dwv[i + u];
          if constexpr (D != 64) {
            int qi = qb + i + u;
            qi = qi < Tq_b ? qi : Tq_b - 1;
            dwe = drop_word(p.drop, drop_wbase(hbase + (uint32_t)qi, (uint32_t)p.Tk, (uint32_t)krow));
          }
          tk[u] = __builtin_amdgcn_ubfe(dwe, fsh, 16) >= thr16 ? dsc : 0.0f;
        }
        const f32x2v arg = f32x2v{sacc[e], sacc[e + 1]} * c1 + (f32x2v{l4[i], l4[i + 1]} + madd);
        f32x2v pe;
        pe.x = __builtin_amdgcn_exp2f(arg.x); pe.y = __builtin_amdgcn_exp2f(arg.y);
        const f32x2v pdv = pe * tk;
        const f32x2v dsv = pe * (f32x2v{dpacc[e], dpacc[e + 1]} * tk - f32x2v{d4[i], d4[i + 1]});   // softmax scale: once, at the end
        pd[e] = pdv.x; pd[e + 1] = pdv.y;
        ds[e] = dsv.x; ds[e + 1] = dsv.y;
      }
    }
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      const bf16x8 pf = pack8(pd + 8 * ss);
      const bf16x8 dsf = pack8(ds + 8 * ss);
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) {
        const bf16x8 dotf = read_tr_frag<D>(doimg, 32 * qt + 16 * ss, 32 * dt, lane);
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dotf, pf, dv[dt], 0, 0, 0);
        const bf16x8 qtf = read_tr_frag<D>(qimg, 32 * qt + 16 * ss, 32 * dt, lane);
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf, dsf, dk[dt], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) dk[dt][e] *= p.scale;
  store_acc_row<D>(p.dk + (kvalid ? grow : 0) * p.lddk + head * D, dk, 1.0f, h, kvalid);
  store_acc_row<D>(p.dv + (kvalid ? grow : 0) * p.lddv + head * D, dv, 1.0f, h, kvalid);
}

// ------------------------------------------------------------------------------------------------
// backward in ONE kernel for the text self-attention (D = 64, up to 256 queries x 256 keys): the dK / dV walk above
// (key on the lane, a wave = one 32-key tile, all query tiles) also produces dQ, so S, P, dP, the mask and the dropout
// words are formed once per score instead of twice (they are ~2/3 of the vector work of either backward kernel).
//   dQ^T[d, q] += sum over the wave's 32 keys of K^T[d, k] dS^T[k, q]: K^T fragments are loop-invariant registers (read
//   once, transposed, from HBM; keys past the end as zeros, so their lanes' dS never counts); dS sits in the accumulator
//   layout [query regs][key lane], which is the operand layout for a reduction over QUERIES (dK) -- for the reduction over
//   keys it goes through a wave-private 2 KiB LDS tile ([key][query] bf16: 4 ds_write_b64 per lane, read back as
//   transposed fragments: no barrier, a wave's LDS accesses execute in order);
//   the eight waves' partial dQ tiles meet in an fp32 LDS accumulator [256 q][64 d (+4 pad)] in WAVE ORDER: a turn word
//   per query tile says which wave may add next (wave 0 stores, wave w adds once the word reads w, then sets w + 1) -- a
//   fixed summation order (the result is rounded to bf16: with LDS float atomics in arrival order the rounding differed
//   from run to run, 3e-3 of the gradient scale at the end of backward) and plain 16-byte read / add / write instead of
//   32 ds_add_f32 per lane and tile (LDS float atomics run at a fraction of the plain rate: the first version of this
//   kernel took 3x the time of the two-kernel path).  Scaled, rounded and written once at the end.
//   delta = rowsum(dO o O) is formed while the images are staged (the two-kernel path got it from the dQ kernel).
// LDS: BwdFusedLds, within 2 KiB of what a CU has: one workgroup per CU -- which the 228-register dK / dV kernel was already
// (two waves per SIMD).
// ------------------------------------------------------------------------------------------------
// What the three one-kernel backward forms put into LDS before their first barrier, per query of the item: -lse log2 e (-inf for
// padded queries: P = 0 there), delta = sum_d dO[q, d] O[q, d] (D / 8 consecutive lanes share a row, 16-byte chunks, reduced by
// log2(D / 8) exchanges), and the INVERTED mask words of every (key tile, query) (bit set = masked), row stride `mstride`.
template <int D>
__device__ __forceinline__ void bwd_stage_row_stats(const AttnBwdParams& p, int b, int head, size_t qbase, int Tq_b, int Tk_b, int qpad_b,
                                                    float* lse_s, float* del_s, uint32_t* mw_s, int mstride, int tid, int nthreads) {
  constexpr int LPR = D / 8;                                    // lanes per row
  for (int i = tid; i < qpad_b; i += nthreads) {
    const size_t stat = ((size_t)b * p.H + head) * p.Tq + i;
    lse_s[i] = i < Tq_b ? -p.lse[stat] * LOG2E : -INFINITY;
  }
  for (int i = tid; i < qpad_b * LPR; i += nthreads) {
    const int row = i / LPR, c = i % LPR;
    float part = 0.f;
    if (row < Tq_b) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(p.dout + (qbase + row) * p.lddo + head * D + 8 * c);
      const u32x4 o = *reinterpret_cast<const u32x4*>(p.o + (qbase + row) * p.ldo + head * D + 8 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        part = fmaf(__uint_as_float(a[e] << 16), __uint_as_float(o[e] << 16), part);
        part = fmaf(__uint_as_float(a[e] & 0xffff0000u), __uint_as_float(o[e] & 0xffff0000u), part);
      }
    }
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) part += __shfl_xor(part, o, 64);
    if (c == 0) del_s[row] = part;
  }
  const int nkt_b = (Tk_b + 31) >> 5;
  const uint32_t* mb = p.mask + (size_t)b * p.mask_b_stride;
  for (int i = tid; i < nkt_b * qpad_b; i += nthreads) {
    const int kt = i / qpad_b, qi = i - kt * qpad_b;
    const int qc = qi < Tq_b ? qi : Tq_b - 1;
    mw_s[kt * mstride + qi] = ~mb[(size_t)qc * p.mask_q_stride + kt] | pad_key_bits(Tk_b, kt);
  }
}

// S and dP of one (32-query tile, 32-key tile) pair in the key-on-the-lane layout (lane (r, h) = key r, register e = query
// key_of_reg-style: 4 consecutive queries per register quad) -> P^T (dropped and scaled: what multiplies dO) and dS^T (before the
// softmax scale), as floats.  q0 = first query of the tile; lse_s (NEGATED, log2 domain) / del_s / mrow (INVERTED mask words of this
// key tile) are LDS arrays indexed by query.  Shared by the three one-kernel backward forms.
struct BwdScoreCtx {
  uint32_t dlane, hbase, halfm, thr16;   // dropout: the lane's part of the counter, (b * H + head) * Tq, words per query row * M1, threshold
  float dsc, c1;                         // keep scale, softmax scale * log2 e
  bool dropping;
};
__device__ __forceinline__ void bwd_score_tile(const AttnBwdParams& p, const BwdScoreCtx& c, const f32x16& sacc, const f32x16& dpacc,
                                               const float* lse_s, const float* del_s, const uint32_t* mrow, int q0, int r, int h,
                                               float (&pd)[16], float (&ds)[16]) {
  constexpr float MOFF = -10000.0f * LOG2E;
  const uint32_t hbase = c.hbase, halfm = c.halfm, dlane = c.dlane, thr16 = c.thr16;
  const float dsc = c.dsc, c1 = c.c1;
  const bool dropping = c.dropping;
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const int qb = q0 + 8 * g4 + 4 * h;   // 4 consecutive queries for registers 4*g4 .. 4*g4+3
    const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_s + qb);
    const f32x4 d4 = *reinterpret_cast<const f32x4*>(del_s + qb);
    const u32x4 w4 = *reinterpret_cast<const u32x4*>(mrow + qb);
    uint32_t dwv[4] = {0u, 0u, 0u, 0u};
    const uint32_t odd = (uint32_t)r & 1u;
    if (dropping) {       // keys k and k^1 share a hash word: each lane of the pair hashes two of the four queries (see attn_bwd_dkv_kernel)
      const uint32_t ua = (hbase + (uint32_t)(q0 + 8 * g4)) * halfm;
      const uint32_t wa = drop_fin(p.drop, dlane + ua);
      const uint32_t wb = drop_fin(p.drop, dlane + ua + 2u * halfm);
      const uint32_t oa = (uint32_t)__builtin_amdgcn_mov_dpp((int)wa, 0xB1, 0xF, 0xF, true);
      const uint32_t ob = (uint32_t)__builtin_amdgcn_mov_dpp((int)wb, 0xB1, 0xF, 0xF, true);
      dwv[0] = odd ? oa : wa; dwv[1] = odd ? wa : oa; dwv[2] = odd ? ob : wb; dwv[3] = odd ? wb : ob;
    }
    const uint32_t fsh = odd << 4;
#pragma unroll
    for (int i = 0; i < 4; i += 2) {
      const int e = 4 * g4 + i;
      f32x2v madd, tk;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const uint32_t mb = (uint32_t)__builtin_amdgcn_sbfe((int)w4[i + u], (uint32_t)r, 1) & __builtin_bit_cast(uint32_t, MOFF);
        madd[u] = __uint_as_float(mb);
        tk[u] = __builtin_amdgcn_ubfe(dwv[i + u], fsh, 16) >= thr16 ? dsc : 0.0f;
      }
      const f32x2v arg = f32x2v{sacc[e], sacc[e + 1]} * c1 + (f32x2v{l4[i], l4[i + 1]} + madd);
      f32x2v pe;
      pe.x = __builtin_amdgcn_exp2f(arg.x); pe.y = __builtin_amdgcn_exp2f(arg.y);
      const f32x2v pdv = pe * tk;
      const f32x2v dsv = pe * (f32x2v{dpacc[e], dpacc[e + 1]} * tk - f32x2v{d4[i], d4[i + 1]});
      pd[e] = pdv.x; pd[e + 1] = pdv.y;
      ds[e] = dsv.x; ds[e + 1] = dsv.y;
    }
  }
}

__device__ __forceinline__ bf16x8 read_tr_tile64(const char* tile, int rowbase, int lane) {
  // [32 rows][32 cols] bf16, 64-byte rows: element j of lane (r, h) = tile[rowbase + 8 (j >> 2) + 4 h + (j & 3)][r]
  const int h = lane >> 5, i = lane & 15, qq = i >> 2, pp = i & 3;
  const int col = 16 * ((lane >> 4) & 1) + 4 * pp;
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  s16x4 part[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int row = rowbase + 8 * jj + 4 * h + qq;
    part[jj] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)LDS_PTR(tile + row * 64 + col * 2));
  }
  s16x8 v = {part[0][0], part[0][1], part[0][2], part[0][3], part[1][0], part[1][1], part[1][2], part[1][3]};
  return __builtin_bit_cast(bf16x8, v);
}

// The same tile with its 8-byte chunks XOR-swizzled by the row (chunk c of row r sits at c ^ ((r >> 2) & 7)): rows r and r + 4 are
// 256 bytes = one pass over the banks apart, so the 8-byte dS^T stores of 16 lanes (rows r .. r + 15, one chunk) hit four bank
// pairs four times each; swizzled they spread over all of them (SQ_LDS_BANK_CONFLICT was 31 % of the LDS-array cycles of the text
// backward, profiles/r5x_attention_text_kernels_pmc.txt).  (A/B builds: UNIMM_ATTN_TILE_SWZ = 0 is the unswizzled tile.)
__device__ __forceinline__ int tile64_swz(int row) { return UNIMM_ATTN_TILE_SWZ ? (row >> 2) & 7 : 0; }
__device__ __forceinline__ bf16x8 read_tr_tile64s(const char* tile, int rowbase, int lane) {
  const int h = lane >> 5, i = lane & 15, qq = i >> 2, pp = i & 3;
  const int chunk = 4 * ((lane >> 4) & 1) + pp;                 // 8-byte chunk = 4 columns
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  s16x4 part[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int row = rowbase + 8 * jj + 4 * h + qq;
    part[jj] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)LDS_PTR(tile + row * 64 + ((chunk ^ tile64_swz(row)) << 3)));
  }
  s16x8 v = {part[0][0], part[0][1], part[0][2], part[0][3], part[1][0], part[1][1], part[1][2], part[1][3]};
  return __builtin_bit_cast(bf16x8, v);
}

// ------------------------------------------------------------------------------------------------
// forward for FEW queries (the co-attention direction whose queries are the 37 regions: D = 128, <= 64 queries x <= 256 keys,
// models/vilbert_dialog.py:701-721).  In attn_fwd_kernel a wave owns a 32-query tile, so two of the eight waves of an item
// compute (64 + 64 MFMAs and 128 scores per lane each) while six only help staging 128 KiB of K / V, one workgroup per CU:
// 6 x 85 us per step.  Here the KEYS are dealt to the waves, as the backward forms do:
//   phase 1   wave w = key tile w.  Its K rows come straight from HBM as MFMA operands (never staged), S^T = K Q^T for both
//             query tiles (query on the lane, the wave's 32 keys in 16 + 16 registers of the lane pair), the tile's row maximum
//             goes to LDS [wave][query]; after a barrier every wave takes the maximum over the eight, forms p = 2^(v - max),
//             leaves its partial row sum in LDS and its P tile (dropped, bf16, [query][32 keys]) for phase 2;
//   phase 2   OUTPUT-stationary: wave (d slice of 32, query tile) = 4 x 2 reads every key tile's P and V^T fragments and owns
//             O^T[32 d][32 q] over all keys -- no accumulator is shared between waves; row sums are added in wave order.
// Same scores, masks (-10000, reference :1418), dropout words and lse as attn_fwd_kernel; sums associate differently (per key
// tile), i.e. results agree to fp32 rounding, and a packed (variable-length) run equals the padded one bit for bit as there.
// LDS: FwdFewq128Lds (one workgroup per CU).  (A/B builds: UNIMM_ATTN_FEWQ_FWD = 0 keeps attn_fwd_kernel<128, 8> for this shape.)
// ------------------------------------------------------------------------------------------------
struct FwdFewq128Lds {
  static constexpr int D = 128, KPAD = 256, QPAD = 64, NW = 8;
  static constexpr int vimg = 0;                                       // [KPAD keys][D] bf16, chunk-swizzled (swz)
  static constexpr int qimg = vimg + KPAD * 2 * D;                     // [QPAD queries][D] bf16, the same
  static constexpr int pt = qimg + QPAD * 2 * D;                       // [key tile][query tile][32 q][32 keys] bf16
  static constexpr int mx_w = pt + NW * 2 * 2048;                      // [wave][QPAD] fp32: the key tile's row maximum
  static constexpr int sm_w = mx_w + NW * QPAD * (int)sizeof(float);   // [wave][QPAD] fp32: its partial row sum
  static constexpr int bytes = sm_w + NW * QPAD * (int)sizeof(float);
  static_assert(bytes <= LDS_CU_BYTES);
  static_assert(lds_aligned16({vimg, qimg, pt}));
};

__global__ __launch_bounds__(512, 1) void attn_fwd_fewq128_kernel(AttnParams p) {
  using L = FwdFewq128Lds;
  constexpr int D = L::D, KPAD = L::KPAD, QPAD = L::QPAD, NW = L::NW;
  drop_resolve(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *vimg = smem + L::vimg, *qimg = smem + L::qimg, *pt = smem + L::pt;
  float *mx_w = reinterpret_cast<float*>(smem + L::mx_w), *sm_w = reinterpret_cast<float*>(smem + L::sm_w);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int item = blockIdx.x;
  const int b = p.order != nullptr ? p.order[item / p.H] : item / p.H, head = item % p.H;
  const int r = lane & 31, h = lane >> 5;
  int Tk_b = p.k_len ? p.k_len[b] : p.Tk;
  Tk_b = Tk_b < KPAD ? Tk_b : KPAD;
  int Tq_b = p.q_len ? p.q_len[b] : p.Tq;
  Tq_b = Tq_b < QPAD ? Tq_b : QPAD;
  const size_t qbase = p.q_off ? (size_t)p.q_off[b] : (size_t)b * p.Tq;
  const size_t kbase = p.k_off ? (size_t)p.k_off[b] : (size_t)b * p.Tk;
  const int kpad_b = (Tk_b + 31) & ~31, qpad_b = (Tq_b + 31) & ~31;
  const int nqt = qpad_b >> 5;
  stage_head<D>(p.v + kbase * p.ldv + head * D, p.ldv, Tk_b, kpad_b, vimg, tid, blockDim.x);
  stage_head<D>(p.q + qbase * p.ldq + head * D, p.ldq, Tq_b, qpad_b, qimg, tid, blockDim.x);

  // ---- phase 1a: this wave's key tile
  const int wt = wave;
  const bool wave_on = wt * 32 < Tk_b;
  int krow = wt * 32 + r;
  if (krow >= Tk_b) krow = Tk_b - 1;
  const bf16_t* kg = p.k + (kbase + krow) * p.ldk + head * D;
  bf16x8 kf[D / 16];
#pragma unroll
  for (int ks = 0; ks < D / 16; ++ks) kf[ks] = *reinterpret_cast<const bf16x8*>(kg + 16 * ks + 8 * h);
  uint32_t mw[2];
  int qrow[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    int q = 32 * qt + r;
    q = q < Tq_b ? q : Tq_b - 1;
    qrow[qt] = q;
    mw[qt] = 32 * wt < p.Tk ? p.mask[(size_t)b * p.mask_b_stride + (size_t)q * p.mask_q_stride + wt] : 0u;   // (ceil(Tk / 32) words a row)
  }
  stage_wait();
  __syncthreads();

  const float c1 = p.scale * LOG2E;
  constexpr float MOFF = -10000.0f * LOG2E;
  f32x16 s[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float mxl = -INFINITY;
    s[qt] = f32x16{};
    if (wave_on && qt < nqt) {
      f32x16 acc = {};
#pragma unroll
      for (int ks = 0; ks < D / 16; ++ks) {
        const bf16x8 qf = read_row_frag<D>(qimg, 32 * qt + r, 2 * ks + h);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf, acc, 0, 0, 0);
      }
      const uint32_t wn = ~(mw[qt] >> (4 * h));               // bit kk set = key kk (+ 4h folded in) of this tile is masked
      const bool partial = 32 * (wt + 1) > Tk_b;               // (wave-uniform) the sequence's last, partial key tile
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        const int kk = (e & 3) + 8 * (e >> 2);
        f32x2v madd;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const uint32_t mb = (uint32_t)__builtin_amdgcn_sbfe((int)wn, kk + u, 1) & __builtin_bit_cast(uint32_t, MOFF);
          madd[u] = __uint_as_float(mb);
          if (partial) madd[u] = (32 * wt + kk + u + 4 * h) < Tk_b ? madd[u] : -INFINITY;   // padded keys do not exist
        }
        const f32x2v v = f32x2v{acc[e], acc[e + 1]} * c1 + madd;
        acc[e] = v.x; acc[e + 1] = v.y;
        mxl = fmaxf(mxl, fmaxf(v.x, v.y));
      }
      s[qt] = acc;
      mxl = fmaxf(mxl, __shfl_xor(mxl, 32, 64));
    }
    if (h == 0) mx_w[wave * QPAD + 32 * qt + r] = mxl;
  }
  __syncthreads();

  // ---- phase 1b: the row maximum over all key tiles, p = 2^(v - max), partial row sums, the wave's P tiles
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float suml = 0.f;
    if (wave_on && qt < nqt) {
      float mx = -INFINITY;
#pragma unroll
      for (int w = 0; w < NW; ++w) mx = fmaxf(mx, mx_w[w * QPAD + 32 * qt + r]);
      f32x2v sum2 = {0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 16; e += 2) {
        const f32x2v a = f32x2v{s[qt][e], s[qt][e + 1]} - mx;
        const float p0 = __builtin_amdgcn_exp2f(a.x), p1 = __builtin_amdgcn_exp2f(a.y);
        s[qt][e] = p0; s[qt][e + 1] = p1;
        sum2 += f32x2v{p0, p1};
      }
      suml = sum2.x + sum2.y;
      suml += __shfl_xor(suml, 32, 64);
      if (p.drop.thr != 0u) {          // the dropout words of attn_fwd_kernel: one hash per two neighbouring keys
        const uint32_t wl = drop_lin(p.drop, drop_wbase(((uint32_t)b * p.H + head) * p.Tq + (uint32_t)qrow[qt], (uint32_t)p.Tk, 0u) + 2u * (uint32_t)h);
#pragma unroll
        for (int e = 0; e < 16; e += 2) {
          const uint32_t w = drop_fin(p.drop, wl + (uint32_t)((32 * wt + key_of_reg(e, 0)) >> 1) * DROP_M1);
          s[qt][e] = drop_keep(p.drop, w, 0u) ? s[qt][e] : 0.0f;
          s[qt][e + 1] = drop_keep(p.drop, w, 1u) ? s[qt][e + 1] : 0.0f;
        }
      }
      char* tile = pt + (wt * 2 + qt) * 2048;                 // [32 q][32 keys] bf16, 64-byte rows, 8-byte chunks swizzled by the row
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        *reinterpret_cast<u32x2*>(tile + r * 64 + (((2 * g4 + h) ^ tile64_swz(r)) << 3)) =
            u32x2{pack2bf(s[qt][4 * g4], s[qt][4 * g4 + 1]), pack2bf(s[qt][4 * g4 + 2], s[qt][4 * g4 + 3])};
    }
    if (h == 0) sm_w[wave * QPAD + 32 * qt + r] = suml;
  }
  __syncthreads();

  // ---- phase 2: wave (dt, qt) owns O^T[32 dt .. 32 dt + 31][query tile qt] over every key tile
  const int dt = wave & 3, qt2 = wave >> 2;
  if (qt2 < nqt) {
    f32x16 o1[1] = {f32x16{}};
    for (int t = 0; t < NW; ++t) {
      if (32 * t >= Tk_b) break;
      const char* tile = pt + (t * 2 + qt2) * 2048;
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        const u32x2 lo = *reinterpret_cast<const u32x2*>(tile + r * 64 + (((4 * ss + h) ^ tile64_swz(r)) << 3));
        const u32x2 hi = *reinterpret_cast<const u32x2*>(tile + r * 64 + (((4 * ss + 2 + h) ^ tile64_swz(r)) << 3));
        const bf16x8 pf = __builtin_bit_cast(bf16x8, u32x4{lo[0], lo[1], hi[0], hi[1]});
        const bf16x8 vf = read_tr_frag<D>(vimg, 32 * t + 16 * ss, 32 * dt, lane);
        o1[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o1[0], 0, 0, 0);
      }
    }
    float mx = -INFINITY, sum = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      mx = fmaxf(mx, mx_w[w * QPAD + 32 * qt2 + r]);
      sum += sm_w[w * QPAD + 32 * qt2 + r];
    }
    const float inv = (p.drop.thr != 0u ? p.drop.scale : 1.0f) / sum;
    const int q = 32 * qt2 + r;
    const bool qvalid = q < Tq_b;
    store_acc_row<32>(p.o + (qbase + (qvalid ? q : 0)) * p.ldo + head * D + 32 * dt, o1, inv, h, qvalid);
    if (dt == 0 && qvalid && h == 0 && p.lse != nullptr) p.lse[((size_t)b * p.H + head) * p.Tq + q] = (mx + __log2f(sum)) * LN2;
  }
}

template <int NQT>
struct BwdFusedLds : BwdDkvLds<64, NQT> {                            // qimg, doimg, lse_s, del_s, mw_s, then
  static constexpr int D = 64, QPAD = NQT * 32;
  static constexpr int AS = D + 4;                                   // accumulator row stride in floats (16-byte accesses of 16 rows cover all banks)
  static constexpr int scr = BwdDkvLds<D, NQT>::bytes;               // [wave][32 keys][32 queries] bf16: the wave's dS^T tile
  static constexpr int acc = scr + 8 * 2048;                         // [QPAD q][AS] fp32: dQ (before the first barrier: the waves' K images)
  static constexpr int turn = acc + QPAD * AS * (int)sizeof(float);  // [NQT] int: the wave whose turn it is to add its partial of that query tile
  static constexpr int bytes = turn + NQT * (int)sizeof(int);
  static_assert(bytes <= LDS_CU_BYTES);
  static_assert(lds_aligned16({scr, acc}) && 8 * 32 * 2 * D <= turn - acc);   // (eight 32-row K images borrow the accumulator)
};

template <int NQT>
__global__ __launch_bounds__(512, 2) void attn_bwd_fused_kernel(AttnBwdParams p) {
  using L = BwdFusedLds<NQT>;
  constexpr int D = L::D, QPAD = L::QPAD, AS = L::AS;
  drop_resolve(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *qimg = smem + L::qimg, *doimg = smem + L::doimg, *scr = smem + L::scr;
  float *lse_s = reinterpret_cast<float*>(smem + L::lse_s), *del_s = reinterpret_cast<float*>(smem + L::del_s);
  uint32_t* mw_s = reinterpret_cast<uint32_t*>(smem + L::mw_s);
  float* acc = reinterpret_cast<float*>(smem + L::acc);
  int* turn = reinterpret_cast<int*>(smem + L::turn);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int item = blockIdx.x;
  const int b = p.order != nullptr ? p.order[item / p.H] : item / p.H, head = item % p.H;
  const int wt = wave;                                          // this wave's 32-key tile
  const int r = lane & 31, h = lane >> 5;

  const int Tq_b = p.q_len ? p.q_len[b] : p.Tq, Tk_b = p.k_len ? p.k_len[b] : p.Tk;
  const size_t qbase = p.q_off ? (size_t)p.q_off[b] : (size_t)b * p.Tq;
  const size_t kbase = p.k_off ? (size_t)p.k_off[b] : (size_t)b * p.Tk;
  const int qpad_b = ((Tq_b + 31) & ~31) < QPAD ? ((Tq_b + 31) & ~31) : QPAD;
  stage_head<D>(p.q + qbase * p.ldq + head * D, p.ldq, Tq_b, qpad_b, qimg, tid, blockDim.x);
  stage_head<D>(p.dout + qbase * p.lddo + head * D, p.lddo, Tq_b, qpad_b, doimg, tid, blockDim.x);
  bwd_stage_row_stats<D>(p, b, head, qbase, Tq_b, Tk_b, qpad_b, lse_s, del_s, mw_s, QPAD, tid, blockDim.x);
  if (tid < NQT) turn[tid] = 0;

  int krow = wt * 32 + r;
  const bool kvalid = krow < Tk_b;
  const bool wave_on = wt * 32 < Tk_b;
  if (!kvalid) krow = Tk_b - 1;
  const size_t grow = kbase + krow;
  const bf16_t* kg = p.k + grow * p.ldk + head * D;
  const bf16_t* vg = p.v + grow * p.ldv + head * D;
  bf16x8 kf[D / 16], vf[D / 16];
#pragma unroll
  for (int ks = 0; ks < D / 16; ++ks) {
    kf[ks] = *reinterpret_cast<const bf16x8*>(kg + 16 * ks + 8 * h);
    vf[ks] = *reinterpret_cast<const bf16x8*>(vg + 16 * ks + 8 * h);
  }
  // K^T fragments of the wave's tile for dQ (fragment (dt, ss): element j of lane (r, h) = K[32 wt + 16 ss + 8 (j >> 2) + 4 h +
  // (j & 3)][32 dt + r]): the row fragments just loaded go through a wave-private image in the (still unused) accumulator
  // area and come back as transposed fragments; rows of keys past the end are written as zeros, so whatever those lanes
  // compute as dS never reaches dQ.  No barrier: a wave's LDS accesses execute in order, and every wave is done with this
  // before the barrier below, after which the area becomes the accumulator.
  bf16x8 ktf[2][2];
  {
    char* kt = reinterpret_cast<char*>(acc) + wave * (32 * 2 * D);
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      const u32x4 v = kvalid ? __builtin_bit_cast(u32x4, kf[ks]) : u32x4{0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4*>(kt + r * (2 * D) + (((2 * ks + h) ^ swz<D>(r)) << 4)) = v;
    }
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      ktf[0][ss] = read_tr_frag<D>(kt, 16 * ss, 0, lane);
      ktf[1][ss] = read_tr_frag<D>(kt, 16 * ss, 32, lane);
    }
  }
  stage_wait();
  __syncthreads();

  f32x16 dk[D / 32], dv[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) { dk[dt] = f32x16{}; dv[dt] = f32x16{}; }
  const uint32_t* mrow = mw_s + wt * QPAD;
  char* ws = scr + wave * 2048;
  const uint32_t hbase = ((uint32_t)b * p.H + head) * (uint32_t)p.Tq;
  const uint32_t halfw = ((uint32_t)p.Tk + 1u) >> 1, halfm = halfw * DROP_M1;
  const uint32_t dlane = drop_lin(p.drop, (4u * (uint32_t)h + ((uint32_t)r & 1u)) * halfw + ((uint32_t)(wt * 32 + r) >> 1));
  const float c1 = p.scale * LOG2E;
  const bool dropping = p.drop.thr != 0u;
  const uint32_t thr16 = dropping ? (p.drop.thr >> 16) : 0u;
  const float dsc = dropping ? p.drop.scale : 1.0f;
  const BwdScoreCtx sctx{dlane, hbase, halfm, thr16, dsc, c1, dropping};

  if (wave_on) {
#pragma unroll 1
  for (int qt = 0; qt < NQT; ++qt) {
    if (32 * qt >= Tq_b) break;
    f32x16 sacc = {}, dpacc = {};
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      const bf16x8 qf = read_row_frag<D>(qimg, 32 * qt + r, 2 * ks + h);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kf[ks], sacc, 0, 0, 0);
      const bf16x8 df = read_row_frag<D>(doimg, 32 * qt + r, 2 * ks + h);
      dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, vf[ks], dpacc, 0, 0, 0);
    }
    float pd[16], ds[16];
    bwd_score_tile(p, sctx, sacc, dpacc, lse_s, del_s, mrow, 32 * qt, r, h, pd, ds);
    // dS^T of this (query tile, key tile) -> the wave's LDS tile: row = key (lane), 4 consecutive queries per store
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
      *reinterpret_cast<u32x2*>(ws + r * 64 + (((2 * g4 + h) ^ tile64_swz(r)) << 3)) =
          u32x2{pack2bf(ds[4 * g4], ds[4 * g4 + 1]), pack2bf(ds[4 * g4 + 2], ds[4 * g4 + 3])};
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      const bf16x8 pf = pack8(pd + 8 * ss);
      const bf16x8 dsf = pack8(ds + 8 * ss);
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt) {
        const bf16x8 dotf = read_tr_frag<D>(doimg, 32 * qt + 16 * ss, 32 * dt, lane);
        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dotf, pf, dv[dt], 0, 0, 0);
        const bf16x8 qtf = read_tr_frag<D>(qimg, 32 * qt + 16 * ss, 32 * dt, lane);
        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf, dsf, dk[dt], 0, 0, 0);
      }
    }
    // dQ^T partial of the tile over this wave's keys, added into the workgroup's accumulator
    f32x16 dqp[2] = {f32x16{}, f32x16{}};
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      const bf16x8 dstf = read_tr_tile64s(ws, 16 * ss, lane);
      dqp[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf[0][ss], dstf, dqp[0], 0, 0, 0);
      dqp[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf[1][ss], dstf, dqp[1], 0, 0, 0);
    }
    // lane (q = r, h) holds d = 32 dt + 8 g + 4 h + {0..3} in registers 4 g .. 4 g + 3 of dqp[dt]
    float* ap = acc + (32 * qt + r) * AS + 4 * h;
    if (wt == 0) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<f32x4*>(ap + 32 * dt + 8 * g) = f32x4{dqp[dt][4 * g], dqp[dt][4 * g + 1], dqp[dt][4 * g + 2], dqp[dt][4 * g + 3]};
    } else {
      while (__hip_atomic_load(turn + qt, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != wt) __builtin_amdgcn_s_sleep(2);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4* a4 = reinterpret_cast<f32x4*>(ap + 32 * dt + 8 * g);
          const f32x4 o = *a4;
          *a4 = f32x4{o[0] + dqp[dt][4 * g], o[1] + dqp[dt][4 * g + 1], o[2] + dqp[dt][4 * g + 2], o[3] + dqp[dt][4 * g + 3]};
        }
    }
    if (lane == 0) __hip_atomic_store(turn + qt, wt + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  }

  if (wave_on) {                                                // (wave-uniform: the lane swap inside needs every lane)
    const bool ok = kvalid;
    store_acc_row<D>(p.dk + (ok ? grow : 0) * p.lddk + head * D, dk, p.scale, h, ok);
    store_acc_row<D>(p.dv + (ok ? grow : 0) * p.lddv + head * D, dv, 1.0f, h, ok);
  }
  __syncthreads();                                              // every wave's dQ partials are in the accumulator
  for (int i = tid; i < qpad_b * 8; i += blockDim.x) {          // 8 lanes = one 128-byte dQ row
    const int q = i >> 3, c = i & 7;
    if (q >= Tq_b) continue;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = acc[q * AS + 8 * c + j] * p.scale;
    *reinterpret_cast<u32x4*>(p.dq + (qbase + q) * p.lddq + head * D + 8 * c) =
        u32x4{pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7])};
  }
}

// ------------------------------------------------------------------------------------------------
// backward in ONE kernel for the co-attention direction whose QUERIES are the 37 regions (and for the image self-attention):
// D = 128, at most 64 queries x 256 keys.  The orientation of attn_bwd_fused_kernel (key on the lane, a wave = one 32-key tile), in
// phases so that it fits 256 registers: the score phase forms S, dP, P, dS of both query tiles ONCE (the two-kernel path formed
// them twice, in kernels of 235 and 256 + 27 spilled registers), leaves dS^T in the wave's LDS tiles and keeps P^T / dS^T as bf16
// MFMA operands (32 registers); dV and dK of the wave's keys then come out one 32-wide slice of D at a time; after a barrier dQ is
// computed output-stationary (a wave = one 32-wide slice of one query tile, over all key tiles: K^T from the tiles' LDS images).
// LDS: BwdFewq128Lds: one workgroup per CU.
// ------------------------------------------------------------------------------------------------
template <int NQT>
struct BwdFewq128Lds : BwdDkvLds<128, NQT> {                       // qimg, doimg, lse_s, del_s, mw_s, then
  static constexpr int D = 128, QPAD = NQT * 32;
  static constexpr int scr = BwdDkvLds<D, NQT>::bytes;              // [wave][query tile][32 keys][32 queries] bf16: the wave's dS^T tiles
  static constexpr int kimgs = scr + 8 * NQT * 2048;                // [wave][32 keys][D] bf16: the wave's K tile, read back transposed for dQ
  static constexpr int bytes = kimgs + 8 * 32 * 2 * D;
  static_assert(bytes <= LDS_CU_BYTES);
  static_assert(lds_aligned16({scr, kimgs}));
};

template <int NQT>
__global__ __launch_bounds__(512, 2) void attn_bwd_fewq128_kernel(AttnBwdParams p) {
  using L = BwdFewq128Lds<NQT>;
  constexpr int D = L::D, QPAD = L::QPAD;
  static_assert(NQT == 2, "the (sequence, head) item's queries are two 32-row tiles: P / dS of both stay in registers for phase 2");
  drop_resolve(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *qimg = smem + L::qimg, *doimg = smem + L::doimg, *scr = smem + L::scr, *kimgs = smem + L::kimgs;
  float *lse_s = reinterpret_cast<float*>(smem + L::lse_s), *del_s = reinterpret_cast<float*>(smem + L::del_s);
  uint32_t* mw_s = reinterpret_cast<uint32_t*>(smem + L::mw_s);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int item = blockIdx.x;
  const int b = p.order != nullptr ? p.order[item / p.H] : item / p.H, head = item % p.H;
  const int wt = wave;                                          // this wave's 32-key tile
  const int r = lane & 31, h = lane >> 5;

  const int Tq_b = p.q_len ? p.q_len[b] : p.Tq, Tk_b = p.k_len ? p.k_len[b] : p.Tk;
  const size_t qbase = p.q_off ? (size_t)p.q_off[b] : (size_t)b * p.Tq;
  const size_t kbase = p.k_off ? (size_t)p.k_off[b] : (size_t)b * p.Tk;
  const int qpad_b = ((Tq_b + 31) & ~31) < QPAD ? ((Tq_b + 31) & ~31) : QPAD;
  stage_head<D>(p.q + qbase * p.ldq + head * D, p.ldq, Tq_b, qpad_b, qimg, tid, blockDim.x);
  stage_head<D>(p.dout + qbase * p.lddo + head * D, p.lddo, Tq_b, qpad_b, doimg, tid, blockDim.x);
  bwd_stage_row_stats<D>(p, b, head, qbase, Tq_b, Tk_b, qpad_b, lse_s, del_s, mw_s, QPAD, tid, blockDim.x);

  int krow = wt * 32 + r;
  const bool kvalid = krow < Tk_b;
  const bool wave_on = wt * 32 < Tk_b;
  if (!kvalid) krow = Tk_b - 1;
  const size_t grow = kbase + krow;
  const bf16_t* kg = p.k + grow * p.ldk + head * D;
  const bf16_t* vg = p.v + grow * p.ldv + head * D;
  bf16x8 kf[D / 16], vf[D / 16];
#pragma unroll
  for (int ks = 0; ks < D / 16; ++ks) {
    kf[ks] = *reinterpret_cast<const bf16x8*>(kg + 16 * ks + 8 * h);
    vf[ks] = *reinterpret_cast<const bf16x8*>(vg + 16 * ks + 8 * h);
  }
  // The wave's K tile also goes to a wave-private LDS image (keys past the end as zeros, so whatever those lanes compute as dS
  // never reaches dQ): dQ reads it back as transposed fragments.  No barrier: a wave's LDS accesses execute in order.
  char* kimg = kimgs + wave * (32 * 2 * D);
#pragma unroll
  for (int ks = 0; ks < D / 16; ++ks) {
    const u32x4 v = kvalid ? __builtin_bit_cast(u32x4, kf[ks]) : u32x4{0u, 0u, 0u, 0u};
    *reinterpret_cast<u32x4*>(kimg + r * (2 * D) + (((2 * ks + h) ^ swz<D>(r)) << 4)) = v;
  }
  stage_wait();
  __syncthreads();

  bf16x8 pfr[NQT][2], dsfr[NQT][2];                             // P^T / dS^T of (query tile, 16-query half) as MFMA operands: phase 2
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt)
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) { pfr[qt][ss] = bf16x8{}; dsfr[qt][ss] = bf16x8{}; }
  const uint32_t* mrow = mw_s + wt * QPAD;
  const uint32_t hbase = ((uint32_t)b * p.H + head) * (uint32_t)p.Tq;
  const uint32_t halfw = ((uint32_t)p.Tk + 1u) >> 1, halfm = halfw * DROP_M1;
  const uint32_t dlane = drop_lin(p.drop, (4u * (uint32_t)h + ((uint32_t)r & 1u)) * halfw + ((uint32_t)(wt * 32 + r) >> 1));
  const float c1 = p.scale * LOG2E;
  const bool dropping = p.drop.thr != 0u;
  const uint32_t thr16 = dropping ? (p.drop.thr >> 16) : 0u;
  const float dsc = dropping ? p.drop.scale : 1.0f;
  const BwdScoreCtx sctx{dlane, hbase, halfm, thr16, dsc, c1, dropping};

  if (wave_on) {
#pragma unroll
  for (int qt = 0; qt < NQT; ++qt) {
    if (32 * qt < Tq_b) {
    f32x16 sacc = {}, dpacc = {};
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      const bf16x8 qf = read_row_frag<D>(qimg, 32 * qt + r, 2 * ks + h);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, kf[ks], sacc, 0, 0, 0);
      const bf16x8 df = read_row_frag<D>(doimg, 32 * qt + r, 2 * ks + h);
      dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, vf[ks], dpacc, 0, 0, 0);
    }
    float pd[16], ds[16];
    bwd_score_tile(p, sctx, sacc, dpacc, lse_s, del_s, mrow, 32 * qt, r, h, pd, ds);
    char* ws = scr + (wave * NQT + qt) * 2048;
    // dS^T of this (query tile, key tile) -> the wave's LDS tile: row = key (lane), 4 consecutive queries per store
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
      *reinterpret_cast<u32x2*>(ws + r * 64 + (((2 * g4 + h) ^ tile64_swz(r)) << 3)) =
          u32x2{pack2bf(ds[4 * g4], ds[4 * g4 + 1]), pack2bf(ds[4 * g4 + 2], ds[4 * g4 + 3])};
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) { pfr[qt][ss] = pack8(pd + 8 * ss); dsfr[qt][ss] = pack8(ds + 8 * ss); }
    }
  }
  }

  // Phase 2: dV = P^T dO and dK = dS^T Q of the wave's 32 keys, one 32-wide slice of D at a time -- 32 accumulator registers
  // alive instead of 2 x 64 through the whole score phase (which is what made this one kernel fit: 2 x 128 + the K / V
  // fragments + a query tile's S, dP, P, dS is 350 registers)
  if (wave_on) {                                                // (wave-uniform: the lane swap inside needs every lane)
    const bool ok = kvalid;
    bf16_t* dkp = p.dk + (ok ? grow : 0) * p.lddk + head * D;
    bf16_t* dvp = p.dv + (ok ? grow : 0) * p.lddv + head * D;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) {
      f32x16 dkc[1] = {f32x16{}}, dvc[1] = {f32x16{}};
#pragma unroll
      for (int qt = 0; qt < NQT; ++qt) {
        if (32 * qt < Tq_b) {
#pragma unroll
          for (int ss = 0; ss < 2; ++ss) {
            const bf16x8 dotf = read_tr_frag<D>(doimg, 32 * qt + 16 * ss, 32 * dt, lane);
            dvc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dotf, pfr[qt][ss], dvc[0], 0, 0, 0);
            const bf16x8 qtf = read_tr_frag<D>(qimg, 32 * qt + 16 * ss, 32 * dt, lane);
            dkc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf, dsfr[qt][ss], dkc[0], 0, 0, 0);
          }
        }
      }
      store_acc_row<32>(dkp + 32 * dt, dkc, p.scale, h, ok);
      store_acc_row<32>(dvp + 32 * dt, dvc, 1.0f, h, ok);
    }
  }
  __syncthreads();                                              // every key tile's dS^T tiles and K image are in LDS
  // dQ, output-stationary: wave w owns the 32-wide slice dt = w & 3 of query tile w >> 2 and walks ALL key tiles -- K^T operand
  // from that tile's K image, dS^T from its tile, both already in LDS.  (The first version added each wave's partial dQ into an
  // fp32 LDS accumulator in wave order and converted it in a last cooperative pass: 16 hand-overs, a barrier and 33 KiB more.)
  {
    const int qt = wave >> 2, dt = wave & 3;
    if (32 * qt < Tq_b) {                                       // (wave-uniform)
      const int nkt = (Tk_b + 31) >> 5;
      f32x16 dqa[1] = {f32x16{}};
#pragma unroll
      for (int kt = 0; kt < 8; ++kt) {
        if (kt < nkt) {
#pragma unroll
          for (int ss = 0; ss < 2; ++ss) {
            const bf16x8 dstf = read_tr_tile64s(scr + (kt * NQT + qt) * 2048, 16 * ss, lane);
            const bf16x8 ktf = read_tr_frag<D>(kimgs + kt * (32 * 2 * D), 16 * ss, 32 * dt, lane);
            dqa[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf, dstf, dqa[0], 0, 0, 0);
          }
        }
      }
      // lane (q = r, h) holds d = 32 dt + 8 g + 4 h + {0..3} in registers 4 g .. 4 g + 3
      const int q = 32 * qt + r;
      const bool ok = q < Tq_b;
      store_acc_row<32>(p.dq + (qbase + (ok ? q : 0)) * p.lddq + head * D + 32 * dt, dqa, p.scale, h, ok);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// ... and for the mirror direction, text queries attending the 37 regions (D = 128, at most 256 queries x 64 keys): the same
// orientation (key on the lane), but a wave is a 32-QUERY tile here and walks the two key tiles.  Its Q / dO rows stay in
// registers as row fragments, K / V are two 16 KiB images shared by the workgroup; dQ of the wave's queries is complete after the
// two key tiles (registers -> global); dK / dV are sums over ALL queries: every wave leaves its P^T / dS^T as MFMA operands in LDS,
// and after one barrier wave w computes ONE output -- a 32-wide slice of dK or dV for both key tiles -- over all query tiles,
// its Q^T / dO^T operand coming straight from global memory through a wave-private 2 KiB tile that is read back transposed
// (phase 2 in the kernel).  LDS: BwdFewk128Lds.  Replaces a dQ kernel (98 us per layer at 240 sequences) and a dK/dV kernel
// (110 us, 312 registers) that formed S, dP, P, dS twice: 148 us.
// ------------------------------------------------------------------------------------------------
struct BwdFewk128Lds {
  static constexpr int D = 128, NKT = 2, KPAD = NKT * 32, QMAX = 256, NQT = QMAX / 32;
  static constexpr int kimg = 0;                                          // [KPAD keys][D] bf16, chunk-swizzled (swz)
  static constexpr int vimg = kimg + KPAD * 2 * D;                        // the same of V
  static constexpr int lse_s = vimg + KPAD * 2 * D;                       // [QMAX] fp32: -lse log2 e
  static constexpr int del_s = lse_s + QMAX * (int)sizeof(float);         // [QMAX] fp32: delta
  static constexpr int mw_s = del_s + QMAX * (int)sizeof(float);          // [key tile][QMAX] inverted mask words
  static constexpr int scr = mw_s + NKT * QMAX * (int)sizeof(uint32_t);   // [wave][dS^T tile of key tile 0 | of key tile 1 | slice tile]: 3 x ([32][32] bf16)
  static constexpr int bfrag = scr + 8 * 6144;                            // [key tile][query tile][dS | P][16-query half]: 1 KiB MFMA operands in register layout
  static constexpr int bytes = bfrag + NKT * NQT * 2 * 2 * 1024;
  static_assert(bytes <= LDS_CU_BYTES);
  static_assert(lds_aligned16({kimg, vimg, lse_s, del_s, mw_s, scr, bfrag}));
};

__global__ __launch_bounds__(512, 2) void attn_bwd_fewk128_kernel(AttnBwdParams p) {
  using L = BwdFewk128Lds;
  constexpr int D = L::D, NKT = L::NKT, KPAD = L::KPAD, QMAX = L::QMAX, NQT = L::NQT;
  drop_resolve(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *kimg = smem + L::kimg, *vimg = smem + L::vimg, *scr = smem + L::scr, *bfrag = smem + L::bfrag;
  float *lse_s = reinterpret_cast<float*>(smem + L::lse_s), *del_s = reinterpret_cast<float*>(smem + L::del_s);
  uint32_t* mw_s = reinterpret_cast<uint32_t*>(smem + L::mw_s);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int item = blockIdx.x;
  const int b = p.order != nullptr ? p.order[item / p.H] : item / p.H, head = item % p.H;
  const int wq = wave;                                          // this wave's 32-query tile
  const int r = lane & 31, h = lane >> 5;

  const int Tq_b = p.q_len ? p.q_len[b] : p.Tq, Tk_b = p.k_len ? p.k_len[b] : p.Tk;
  const size_t qbase = p.q_off ? (size_t)p.q_off[b] : (size_t)b * p.Tq;
  const size_t kbase = p.k_off ? (size_t)p.k_off[b] : (size_t)b * p.Tk;
  const int qpad_b = ((Tq_b + 31) & ~31) < QMAX ? ((Tq_b + 31) & ~31) : QMAX;
  const int kpad_b = ((Tk_b + 31) & ~31) < KPAD ? ((Tk_b + 31) & ~31) : KPAD;
  stage_head<D>(p.k + kbase * p.ldk + head * D, p.ldk, Tk_b, kpad_b, kimg, tid, blockDim.x);
  stage_head<D>(p.v + kbase * p.ldv + head * D, p.ldv, Tk_b, kpad_b, vimg, tid, blockDim.x);
  bwd_stage_row_stats<D>(p, b, head, qbase, Tq_b, Tk_b, qpad_b, lse_s, del_s, mw_s, QMAX, tid, blockDim.x);

  int qrow = wq * 32 + r;
  const bool qvalid = qrow < Tq_b;
  const bool wave_on = wq * 32 < Tq_b;
  if (!qvalid) qrow = Tq_b - 1;
  const size_t grow = qbase + qrow;
  const bf16_t* qg = p.q + grow * p.ldq + head * D;
  const bf16_t* dg = p.dout + grow * p.lddo + head * D;
  bf16x8 qf[D / 16], dof[D / 16];                               // row fragments of the wave's queries: lane (r, h) = row r, columns 16 ks + 8 h ..
#pragma unroll
  for (int ks = 0; ks < D / 16; ++ks) {
    qf[ks] = *reinterpret_cast<const bf16x8*>(qg + 16 * ks + 8 * h);
    dof[ks] = *reinterpret_cast<const bf16x8*>(dg + 16 * ks + 8 * h);
  }
  stage_wait();
  __syncthreads();

  char* wsb = scr + wave * 6144;
  const uint32_t hbase = ((uint32_t)b * p.H + head) * (uint32_t)p.Tq;
  const uint32_t halfw = ((uint32_t)p.Tk + 1u) >> 1, halfm = halfw * DROP_M1;
  const float c1 = p.scale * LOG2E;
  const bool dropping = p.drop.thr != 0u;
  const uint32_t thr16 = dropping ? (p.drop.thr >> 16) : 0u;
  const float dsc = dropping ? p.drop.scale : 1.0f;

  if (wave_on) {
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    if (32 * kt < Tk_b) {
    const uint32_t* mrow = mw_s + kt * QMAX;
    char* ws = wsb + kt * 2048;
    const uint32_t dlane = drop_lin(p.drop, (4u * (uint32_t)h + ((uint32_t)r & 1u)) * halfw + ((uint32_t)(kt * 32 + r) >> 1));
    const BwdScoreCtx sctx{dlane, hbase, halfm, thr16, dsc, c1, dropping};
    f32x16 sacc = {}, dpacc = {};
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      const bf16x8 kfr = read_row_frag<D>(kimg, 32 * kt + r, 2 * ks + h);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[ks], kfr, sacc, 0, 0, 0);
      const bf16x8 vfr = read_row_frag<D>(vimg, 32 * kt + r, 2 * ks + h);
      dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dof[ks], vfr, dpacc, 0, 0, 0);
    }
    float pd[16], ds[16];
    bwd_score_tile(p, sctx, sacc, dpacc, lse_s, del_s, mrow, 32 * wq, r, h, pd, ds);
    // dS^T of this (query tile, key tile) -> the wave's LDS tile: row = key (lane), 4 consecutive queries per store
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4)
      *reinterpret_cast<u32x2*>(ws + r * 64 + (((2 * g4 + h) ^ tile64_swz(r)) << 3)) =
          u32x2{pack2bf(ds[4 * g4], ds[4 * g4 + 1]), pack2bf(ds[4 * g4 + 2], ds[4 * g4 + 3])};
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) {
      // P^T / dS^T of this (key tile, query tile) as MFMA operands, in register layout (16 bytes per lane): phase 2 reads them back
      char* f = bfrag + ((((kt * NQT + wq) * 2) * 2 + ss) << 10) + lane * 16;
      *reinterpret_cast<u32x4*>(f) = __builtin_bit_cast(u32x4, pack8(ds + 8 * ss));
      *reinterpret_cast<u32x4*>(f + 2048) = __builtin_bit_cast(u32x4, pack8(pd + 8 * ss));
    }
    }
  }
  // dQ^T of the wave's queries = K^T dS^T over both key tiles (lane = query, registers = D values): after the score phase, whose
  // S / dP / P / dS registers are dead by now
  f32x16 dqp[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) dqp[dt] = f32x16{};
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    if (32 * kt < Tk_b) {
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        const bf16x8 dstf = read_tr_tile64s(wsb + kt * 2048, 16 * ss, lane);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt)
          dqp[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(read_tr_frag<D>(kimg, 32 * kt + 16 * ss, 32 * dt, lane), dstf, dqp[dt], 0, 0, 0);
      }
    }
  }
  store_acc_row<D>(p.dq + (qvalid ? grow : 0) * p.lddq + head * D, dqp, p.scale, h, qvalid);

  }
  __syncthreads();                                              // every query tile's P^T / dS^T operands are in LDS

  // Phase 2, output-stationary: wave w owns ONE output, the 32-wide slice dt = w & 3 of dK (w < 4) or dV (w >= 4) for both key
  // tiles, and walks ALL query tiles: A = the slice of Q^T (dO^T) -- 32 rows x 64 bytes straight from global memory (L2: phase 1
  // just read those rows) through the wave's 2 KiB tile, read back transposed -- B = the tile's dS^T (P^T) operand from LDS.  No
  // accumulator is shared between waves (the first version added every wave's partials into two LDS accumulators in wave order:
  // 16 hand-overs per wave with nothing to compute between them, ~1/3 of the item's time), and the waves whose query tile does
  // not exist work here too.  (The phase-1 blocks above are inside `if (wave_on)`; this one is not.)
  {
    const int which = wave >> 2, dt = wave & 3;
    const int nqt = (Tq_b + 31) >> 5;
    const bf16_t* src = (which == 0 ? p.q : p.dout) + head * D + 32 * dt + 16 * (lane & 1);
    const size_t ld = which == 0 ? (size_t)p.ldq : (size_t)p.lddo;
    u32x4 rg[NQT][2];                                           // the slice rows of every query tile: lane = (row = lane >> 1, 32-byte half = lane & 1)
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      int row = 32 * qt + (lane >> 1);
      row = row < Tq_b ? row : Tq_b - 1;                        // (rows past the end: their P / dS are zero, any finite values do)
      const bf16_t* g = src + (qbase + row) * ld;
      if (qt < nqt) {
        rg[qt][0] = *reinterpret_cast<const u32x4*>(g);
        rg[qt][1] = *reinterpret_cast<const u32x4*>(g + 8);
      } else {
        rg[qt][0] = u32x4{0u, 0u, 0u, 0u}; rg[qt][1] = u32x4{0u, 0u, 0u, 0u};
      }
    }
    f32x16 oacc[NKT] = {f32x16{}, f32x16{}};
    char* ws2 = scr + wave * 6144 + 4096;
#pragma unroll
    for (int qt = 0; qt < NQT; ++qt) {
      if (qt < nqt) {
        char* t = ws2 + (lane >> 1) * 64 + (lane & 1) * 32;
        *reinterpret_cast<u32x4*>(t) = rg[qt][0];
        *reinterpret_cast<u32x4*>(t + 16) = rg[qt][1];
        const bf16x8 tf0 = read_tr_tile64(ws2, 0, lane), tf1 = read_tr_tile64(ws2, 16, lane);
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
          if (32 * kt < Tk_b) {
            const char* f = bfrag + ((((kt * NQT + qt) * 2 + which) * 2) << 10) + lane * 16;
            oacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf0, *reinterpret_cast<const bf16x8*>(f), oacc[kt], 0, 0, 0);
            oacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tf1, *reinterpret_cast<const bf16x8*>(f + 1024), oacc[kt], 0, 0, 0);
          }
        }
      }
    }
    // lane (key = r, h) holds d = 32 dt + 8 g + 4 h + {0..3} in registers 4 g .. 4 g + 3: the 64-byte slice of the key's row
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      if (32 * kt < Tk_b) {                                       // (workgroup-uniform: the lane swap inside needs every lane)
        const int key = 32 * kt + r;
        const bool ok = key < Tk_b;
        bf16_t* dst = (which == 0 ? p.dk + (kbase + (ok ? key : 0)) * p.lddk : p.dv + (kbase + (ok ? key : 0)) * p.lddv) + head * D + 32 * dt;
        const f32x16 one[1] = {oacc[kt]};
        store_acc_row<32>(dst, one, which == 0 ? p.scale : 1.0f, h, ok);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward of the SPLICED text self-attention (unimm_attn_spliced_fwd: the private query rows of a sequence attend their own
// rows and their group's shared key/value segment, D = 64, at most 32 private rows, at most 256 key positions).
// The orientation of attn_bwd_fused_kernel, one workgroup per (group, head): wave w holds tile w of the SHARED segment (32 keys on
// the lanes: K / V images in LDS, the fp32 dK / dV accumulators in registers for the whole walk) and wave 7 the current sequence's
// <= 32 PRIVATE keys (when the segment has an eighth tile, both: its shared accumulators are parked in LDS meanwhile).  The workgroup walks the group's sequences: a sequence's Q / dO rows,
// -lse, delta and the mask words of every key tile (re-aligned from key POSITIONS to the tile's keys) are staged in LDS, every
// wave forms S, dP, P, dS of its tile against the one query tile, adds into its dK / dV and leaves dS^T in its LDS tile; two
// waves then form dQ^T over all key tiles, in tile order.  The private wave stores its dK / dV per sequence; the shared tiles are
// rounded to bf16 ONCE, after the walk (with `accumulate`, together with what the rows already hold).  No atomics:
// the result does not depend on how workgroups are scheduled.  Registers: 256, 4 of them spilled (20 bytes of scratch per lane).
// LDS: SplicedBwdLds (Q / dO images, row words, dS^T tiles, K and V images, parking): one workgroup per CU.
// ------------------------------------------------------------------------------------------------
struct AttnSplBwdParams {
  AttnBwdParams b;
  const int* ks_off; const int* ks_len; int ks_ins;
  const int* g_first; const int* g_seq; int G;
  int accumulate;
};

// 32 mask bits of one row from key position pos0 on (words past the row's nw words read as 0)
__device__ __forceinline__ uint32_t mask_bits_at(const uint32_t* mr, int nw, int pos0) {
  const int w = pos0 >> 5, sh = pos0 & 31;
  const uint32_t lo = w < nw ? mr[w] : 0u, hi = w + 1 < nw ? mr[w + 1] : 0u;
  return sh == 0 ? lo : (lo >> sh) | (hi << (32 - sh));
}

// bwd_score_tile for a tile whose lane holds the key at POSITION kpos (any parity: every lane hashes its own words);
// lin0 = linear hash stage of (query 0, kpos), halfm = words per query row * M1, fsh = 16 (kpos & 1)
__device__ __forceinline__ void spl_score_tile(const DropoutArg& drop, uint32_t lin0, uint32_t halfm, uint32_t fsh, uint32_t thr16,
                                               float dsc, float c1, bool dropping, const f32x16& sacc, const f32x16& dpacc,
                                               const float* lse_s, const float* del_s, const uint32_t* mrow, int r, int h,
                                               float (&pd)[16], float (&ds)[16]) {
  constexpr float MOFF = -10000.0f * LOG2E;
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const int qb = 8 * g4 + 4 * h;        // 4 consecutive queries for registers 4*g4 .. 4*g4+3
    const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_s + qb);
    const f32x4 d4 = *reinterpret_cast<const f32x4*>(del_s + qb);
    const u32x4 w4 = *reinterpret_cast<const u32x4*>(mrow + qb);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = 4 * g4 + i;
      const uint32_t mb = (uint32_t)__builtin_amdgcn_sbfe((int)w4[i], (uint32_t)r, 1) & __builtin_bit_cast(uint32_t, MOFF);
      float tk = dsc;
      if (dropping) {
        const uint32_t w = drop_fin(drop, lin0 + (uint32_t)(qb + i) * halfm);
        tk = __builtin_amdgcn_ubfe(w, fsh, 16) >= thr16 ? dsc : 0.0f;
      }
      const float pe = __builtin_amdgcn_exp2f(sacc[e] * c1 + (l4[i] + __uint_as_float(mb)));
      pd[e] = pe * tk;
      ds[e] = pe * (dpacc[e] * tk - d4[i]);
    }
  }
}

// LDS of this kernel (QT = 1) and of attn_spliced_wide_bwd_kernel (QT = 2): QT = query tiles, and private key tiles, of a sequence
template <int QT>
struct SplicedBwdLds {
  static constexpr int D = 64, PT = 8, NT = PT + QT, IMG = 32 * 2 * D;     // key tiles: PT shared, then the private ones; IMG: bytes of a 32-row image
  static constexpr int qimg = 0;                                           // [QT query tiles][32][D] bf16, chunk-swizzled (swz)
  static constexpr int doimg = qimg + QT * IMG;                            // the same of dO
  static constexpr int lse_s = doimg + QT * IMG;                           // [32 QT queries] fp32: -lse log2 e
  static constexpr int del_s = lse_s + 32 * QT * (int)sizeof(float);       // [32 QT queries] fp32: delta
  static constexpr int mw_s = del_s + 32 * QT * (int)sizeof(float);        // [key tile][32 QT queries] INVERTED mask words of the tile's keys
  static constexpr int scr = mw_s + NT * 32 * QT * (int)sizeof(uint32_t);  // [key tile][query tile][32 keys][32 queries] bf16 dS^T
  static constexpr int kimg = scr + NT * QT * 2048;                        // [PT shared tiles + 2 buffers (alternating) x QT private tiles][32 keys][D] bf16
  static constexpr int vimg = kimg + (PT + 2 * QT) * IMG;                  // [PT shared tiles + the private tile (at work)][32 keys][D] bf16
  static constexpr int park = vimg + (PT + 1) * IMG;                       // [64 registers][64 lanes] fp32: see `both` in the kernels
  static constexpr int bytes = park + 64 * 64 * (int)sizeof(float);
  static_assert(bytes <= LDS_CU_BYTES);
  static_assert(lds_aligned16({qimg, doimg, lse_s, del_s, mw_s, scr, kimg, vimg}));
};

__global__ __launch_bounds__(512, 2) void attn_spliced_bwd_kernel(AttnSplBwdParams sp) {
  using L = SplicedBwdLds<1>;
  constexpr int D = L::D, NT = L::NT, PT = L::PT, PW = 7, IMG = L::IMG;   // PT: the private tile, PW: its wave
  AttnBwdParams& p = sp.b;
  drop_resolve(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *qimg = smem + L::qimg, *doimg = smem + L::doimg, *scr = smem + L::scr, *kimg = smem + L::kimg, *vimg = smem + L::vimg;
  float *lse_s = reinterpret_cast<float*>(smem + L::lse_s), *del_s = reinterpret_cast<float*>(smem + L::del_s);
  uint32_t* mw_s = reinterpret_cast<uint32_t*>(smem + L::mw_s);
  float* park = reinterpret_cast<float*>(smem + L::park);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = blockIdx.x / p.H, head = blockIdx.x % p.H;
  const int r = lane & 31, h = lane >> 5;
  const int nw = (p.Tk + 31) >> 5;

  int m0 = sp.g_first[g], m1 = sp.g_first[g + 1];
  m0 = m0 < 0 ? 0 : m0;
  m1 = m1 > p.B ? p.B : m1;
  // the group's segment: that of its first member that names one
  int slen = 0;
  size_t soff = 0;
  for (int m = m0; m < m1 && slen == 0; ++m) {
    const int b = sp.g_seq[m];
    if (b < 0 || b >= p.B) continue;
    const int l = sp.ks_len[b];
    if (l > 0) { slen = l < 256 ? l : 256; soff = (size_t)sp.ks_off[b]; }
  }
  const int nst = (slen + 31) >> 5;                             // shared key tiles
  const bool is_priv = wave == PW;
  // A segment of more than 224 rows has a tile for the private wave too.  That wave then runs both passes per sequence, and its
  // shared accumulators wait in LDS while the registers serve the private tile.
  const bool both = is_priv && nst > PW;

  // The wave's 32 keys (rows first .. first + n - 1 of k / v) as LDS images: K / V row fragments for S and dP, K^T for dQ.  Rows past
  // n are zero, so what those lanes compute never reaches dQ.  (A wave reads its own images without a barrier: its LDS accesses
  // execute in order.)
  auto load_keys = [&](size_t first, int n, char* kt, char* vt) {
    const bool ok = r < n;
    const size_t row = first + (ok ? r : n - 1);
    const bf16_t* kg = p.k + row * p.ldk + head * D;
    const bf16_t* vg = p.v + row * p.ldv + head * D;
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      u32x4 kv = *reinterpret_cast<const u32x4*>(kg + 16 * ks + 8 * h);
      u32x4 vv = *reinterpret_cast<const u32x4*>(vg + 16 * ks + 8 * h);
      if (!ok) { kv = u32x4{0u, 0u, 0u, 0u}; vv = kv; }
      *reinterpret_cast<u32x4*>(kt + r * (2 * D) + (((2 * ks + h) ^ swz<D>(r)) << 4)) = kv;
      *reinterpret_cast<u32x4*>(vt + r * (2 * D) + (((2 * ks + h) ^ swz<D>(r)) << 4)) = vv;
    }
  };
  const bool shared_on = wave < nst;
  const int sn = slen - 32 * wave < 32 ? slen - 32 * wave : 32;   // (shared waves) keys of the wave's tile
  if (shared_on) load_keys(soff + 32 * wave, sn, kimg + wave * IMG, vimg + wave * IMG);

  f32x16 dk[D / 32], dv[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) { dk[dt] = f32x16{}; dv[dt] = f32x16{}; }
  const uint32_t halfw = ((uint32_t)p.Tk + 1u) >> 1, halfm = halfw * DROP_M1;
  const float c1 = p.scale * LOG2E;
  const bool dropping = p.drop.thr != 0u;
  const uint32_t thr16 = dropping ? (p.drop.thr >> 16) : 0u;
  const float dsc = dropping ? p.drop.scale : 1.0f;
  int pbuf = 0;                                                 // which private K image this sequence uses

#pragma unroll 1
  for (int m = m0; m < m1; ++m) {
    const int b = sp.g_seq[m];
    if (b < 0 || b >= p.B) continue;
    int ql = p.q_len[b], kl = p.k_len[b];
    ql = ql < 32 ? ql : 32; ql = ql < p.Tq ? ql : p.Tq;
    kl = kl < 0 ? 0 : (kl < 32 ? kl : 32);
    const bool has_s = sp.ks_len[b] > 0 && slen > 0;
    const int Ts = has_s ? slen : 0;
    if (ql <= 0 || kl + Ts <= 0) continue;                       // (workgroup-uniform)
    const int ins = sp.ks_ins < kl ? sp.ks_ins : kl;             // private rows ahead of the segment
    const size_t qbase = (size_t)p.q_off[b], kbase = (size_t)p.k_off[b];
    const int nsh = has_s ? nst : 0;
    const bool s_on = wave < nsh, p_on = is_priv && kl > 0;
    pbuf ^= 1;

    // ---- stage the sequence's query tile
    stage_head<D>(p.q + qbase * p.ldq + head * D, p.ldq, ql, 32, qimg, tid, blockDim.x);
    stage_head<D>(p.dout + qbase * p.lddo + head * D, p.lddo, ql, 32, doimg, tid, blockDim.x);
    if (tid >= 256) {                                            // delta = rowsum(dO o O): 8 lanes share a row
      const int i = tid - 256, row = i >> 3, c = i & 7;
      float part = 0.f;
      if (row < ql) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(p.dout + (qbase + row) * p.lddo + head * D + 8 * c);
        const u32x4 o = *reinterpret_cast<const u32x4*>(p.o + (qbase + row) * p.ldo + head * D + 8 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          part = fmaf(__uint_as_float(a[e] << 16), __uint_as_float(o[e] << 16), part);
          part = fmaf(__uint_as_float(a[e] & 0xffff0000u), __uint_as_float(o[e] & 0xffff0000u), part);
        }
      }
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) part += __shfl_xor(part, o, 64);
      if (c == 0) del_s[row] = part;
      if (i < 32) lse_s[i] = i < ql ? -p.lse[((size_t)b * p.H + head) * p.Tq + i] * LOG2E : -INFINITY;
    }
    if (tid < NT * 32) {                                         // mask words of (tile, query), in the tile's key order
      const int t = tid >> 5, qi = tid & 31;
      const int qc = qi < ql ? qi : ql - 1;
      const uint32_t* mr = p.mask + (size_t)b * p.mask_b_stride + (size_t)qc * p.mask_q_stride;
      uint32_t bits, pad;
      if (t < PT) {                                              // shared keys 32 t ..: positions ins + 32 t ..
        bits = mask_bits_at(mr, nw, ins + 32 * t);
        const int n = Ts - 32 * t;
        pad = n >= 32 ? 0u : (n <= 0 ? ~0u : ~0u << n);
      } else {                                                   // private key i: position i below ins, else i + Ts
        const uint32_t lo = mask_bits_at(mr, nw, 0), hi = mask_bits_at(mr, nw, ins + Ts);
        bits = ins >= 32 ? lo : ((lo & ((1u << ins) - 1u)) | (hi << ins));
        pad = kl >= 32 ? 0u : ~0u << kl;
      }
      mw_s[t * 32 + qi] = ~bits | pad;
    }
    if (p_on) load_keys(kbase, kl, kimg + (PT + pbuf) * IMG, vimg + PT * IMG);
    stage_wait();
    __syncthreads();

    // S, dP, P, dS of key tile t (its key on the lane, at position kpos) against the query tile; dS^T to the tile's LDS image
    // (row = key, 4 consecutive queries per store: what dQ is formed from), dV and dK into the wave's accumulators
    auto tile_pass = [&](int t, const char* kt, int kpos) {
      const char* vt = vimg + t * IMG;
      char* ws = scr + t * 2048;
      const uint32_t lin0 = drop_lin(p.drop, ((uint32_t)b * p.H + head) * (uint32_t)p.Tq * halfw + ((uint32_t)kpos >> 1));
      f32x16 sacc = {}, dpacc = {};
#pragma unroll
      for (int ks = 0; ks < D / 16; ++ks) {
        const bf16x8 qf = read_row_frag<D>(qimg, r, 2 * ks + h);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, read_row_frag<D>(kt, r, 2 * ks + h), sacc, 0, 0, 0);
        const bf16x8 df = read_row_frag<D>(doimg, r, 2 * ks + h);
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, read_row_frag<D>(vt, r, 2 * ks + h), dpacc, 0, 0, 0);
      }
      float pd[16], ds[16];
      spl_score_tile(p.drop, lin0, halfm, ((uint32_t)kpos & 1u) << 4, thr16, dsc, c1, dropping, sacc, dpacc, lse_s, del_s,
                     mw_s + t * 32, r, h, pd, ds);
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        *reinterpret_cast<u32x2*>(ws + r * 64 + (((2 * g4 + h) ^ tile64_swz(r)) << 3)) =
            u32x2{pack2bf(ds[4 * g4], ds[4 * g4 + 1]), pack2bf(ds[4 * g4 + 2], ds[4 * g4 + 3])};
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        const bf16x8 pf = pack8(pd + 8 * ss);
        const bf16x8 dsf = pack8(ds + 8 * ss);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) {
          const bf16x8 dotf = read_tr_frag<D>(doimg, 16 * ss, 32 * dt, lane);
          dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dotf, pf, dv[dt], 0, 0, 0);
          const bf16x8 qtf = read_tr_frag<D>(qimg, 16 * ss, 32 * dt, lane);
          dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf, dsf, dk[dt], 0, 0, 0);
        }
      }
    };
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {                       // (one copy of the code: the two passes inlined do not fit the registers)
      const bool priv = pass == 1;
      if (priv ? !p_on : !s_on) continue;                        // (wave-uniform: the lane swap of the stores needs every lane)
      if (priv) {
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            if (both) { park[(32 * dt + e) * 64 + lane] = dk[dt][e]; park[(32 * dt + 16 + e) * 64 + lane] = dv[dt][e]; }
            dk[dt][e] = 0.f; dv[dt][e] = 0.f;
          }
      }
      const int t = priv ? PT : wave;
      tile_pass(t, kimg + (priv ? PT + pbuf : wave) * IMG, priv ? (r < ins ? r : r + Ts) : ins + 32 * wave + r);
      if (priv) {
        const bool ok = r < kl;
        store_acc_row<D>(p.dk + (kbase + (ok ? r : 0)) * p.lddk + head * D, dk, p.scale, h, ok);
        store_acc_row<D>(p.dv + (kbase + (ok ? r : 0)) * p.lddv + head * D, dv, 1.0f, h, ok);
        if (both) {
#pragma unroll
          for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) { dk[dt][e] = park[(32 * dt + e) * 64 + lane]; dv[dt][e] = park[(32 * dt + 16 + e) * 64 + lane]; }
        }
      }
    }
    __syncthreads();                                             // every tile's dS^T is in LDS
    // ---- dQ^T, output-stationary: wave 5 + dt owns the 32-wide slice dt of D over every key tile, in tile order (the K^T
    // fragments are transposed reads of the tiles' K images).  The other waves go on to stage the next sequence: nothing read
    // here is rewritten before the next staging barrier, the private K image alternates.
    if (wave == 5 || wave == 6) {
      const int dt = wave - 5;
      f32x16 dq1[1] = {f32x16{}};
      const int ntile = nsh + (kl > 0 ? 1 : 0);
      for (int i = 0; i < ntile; ++i) {
        const int t = i < nsh ? i : PT;
        const char* ki = kimg + (t == PT ? PT + pbuf : t) * IMG;
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
          const bf16x8 ktf = read_tr_frag<D>(ki, 16 * ss, 32 * dt, lane);
          const bf16x8 dstf = read_tr_tile64s(scr + t * 2048, 16 * ss, lane);
          dq1[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf, dstf, dq1[0], 0, 0, 0);
        }
      }
      const bool ok = r < ql;
      store_acc_row<32>(p.dq + (qbase + (ok ? r : 0)) * p.lddq + head * D + 32 * dt, dq1, p.scale, h, ok);
    }
  }

  if (shared_on) {                                               // the segment's rows: one rounding of the fp32 sums
    const bool ok = r < sn;
    bf16_t* dkg = p.dk + (soff + 32 * wave + (ok ? r : 0)) * p.lddk + head * D;
    bf16_t* dvg = p.dv + (soff + 32 * wave + (ok ? r : 0)) * p.lddv + head * D;
    if (!sp.accumulate) {
      store_acc_row<D>(dkg, dk, p.scale, h, ok);
      store_acc_row<D>(dvg, dv, 1.0f, h, ok);
    } else if (ok) {                                             // ... together with what the rows hold
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
          const int d0 = 32 * dt + 8 * gg + 4 * h;               // registers 4 gg .. 4 gg + 3 = columns d0 .. d0 + 3
          u32x2* pk = reinterpret_cast<u32x2*>(dkg + d0);
          u32x2* pv = reinterpret_cast<u32x2*>(dvg + d0);
          const u32x2 hk = *pk, hv = *pv;
          *pk = u32x2{pack2bf(fmaf(dk[dt][4 * gg], p.scale, __uint_as_float(hk[0] << 16)),
                              fmaf(dk[dt][4 * gg + 1], p.scale, __uint_as_float(hk[0] & 0xffff0000u))),
                      pack2bf(fmaf(dk[dt][4 * gg + 2], p.scale, __uint_as_float(hk[1] << 16)),
                              fmaf(dk[dt][4 * gg + 3], p.scale, __uint_as_float(hk[1] & 0xffff0000u)))};
          *pv = u32x2{pack2bf(dv[dt][4 * gg] + __uint_as_float(hv[0] << 16), dv[dt][4 * gg + 1] + __uint_as_float(hv[0] & 0xffff0000u)),
                      pack2bf(dv[dt][4 * gg + 2] + __uint_as_float(hv[1] << 16), dv[dt][4 * gg + 3] + __uint_as_float(hv[1] & 0xffff0000u))};
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The same for up to 64 private rows per sequence (unimm_attn_spliced_wide_bwd): two query tiles and two private key tiles.
// Same orientation and the same walk, one workgroup per (group, head), 8 shared key tiles on waves 0 .. 7, the private tiles on
// wave 7 (the second one on wave 6 when that wave has no shared tile).  What changes:
//   * BOTH query tiles of a sequence are staged at once (64-row Q / dO images, 64 -lse / delta values, mask words of every
//     (key tile, query)), so a sequence still costs one staging and two barriers.  A shared wave runs its tile against query
//     tile 0 then 1 and adds both into its accumulators; a private wave takes its key tiles one after the other, each against
//     both query tiles, and stores the tile's rows before it starts the next: 64 accumulator registers serve both, and a private
//     row is still rounded once.  (When the segment has an eighth tile the wave's shared accumulators wait in LDS as before.)
//   * every (key tile, query tile) pair leaves its own dS^T tile; waves 3 .. 6 form dQ^T of (query tile, 32-wide slice of D) over
//     the shared tiles then the private tiles, in tile order.
//   * the V rows of a private tile are read by their own wave only, so ONE private V image serves both tiles: the wave loads it
//     right before the tile's passes (its own LDS accesses execute in order).
// LDS: SplicedBwdLds<2>, within 1 KiB of what a CU has: one workgroup per CU, as the narrow kernel's layout already gives.
// __launch_bounds__(512, 1) asks for one wave per SIMD at least, which the LDS already settles; it buys no registers: the workgroup's
// eight waves are two per SIMD, so 256 is the most a wave can get, and the kernel takes 256 with 63 spilled (256 bytes of scratch per lane).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 1) void attn_spliced_wide_bwd_kernel(AttnSplBwdParams sp) {
  using L = SplicedBwdLds<2>;
  constexpr int D = L::D, NT = L::NT, PT = L::PT, PW = 7, IMG = L::IMG;
  AttnBwdParams& p = sp.b;
  drop_resolve(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *qimg = smem + L::qimg, *doimg = smem + L::doimg, *scr = smem + L::scr, *kimg = smem + L::kimg, *vimg = smem + L::vimg;
  float *lse_s = reinterpret_cast<float*>(smem + L::lse_s), *del_s = reinterpret_cast<float*>(smem + L::del_s);
  uint32_t* mw_s = reinterpret_cast<uint32_t*>(smem + L::mw_s);
  float* park = reinterpret_cast<float*>(smem + L::park);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int g = blockIdx.x / p.H, head = blockIdx.x % p.H;
  const int r = lane & 31, h = lane >> 5;
  const int nw = (p.Tk + 31) >> 5;

  int m0 = sp.g_first[g], m1 = sp.g_first[g + 1];
  m0 = m0 < 0 ? 0 : m0;
  m1 = m1 > p.B ? p.B : m1;
  int slen = 0;
  size_t soff = 0;
  for (int m = m0; m < m1 && slen == 0; ++m) {
    const int b = sp.g_seq[m];
    if (b < 0 || b >= p.B) continue;
    const int l = sp.ks_len[b];
    if (l > 0) { slen = l < 256 ? l : 256; soff = (size_t)sp.ks_off[b]; }
  }
  const int nst = (slen + 31) >> 5;
  // Private key tile 0 is wave 7's.  Tile 1 is wave 6's when that wave has no shared tile (a segment of at most 192 rows): the two
  // tiles then run side by side, and its V image takes the wave's unused shared slot.  Otherwise wave 7 takes both in turn.
  const bool split = nst <= PW - 1;
  const bool is_priv = wave == PW || (split && wave == PW - 1);
  const int pt0 = wave == PW ? 0 : 1, pt1 = (wave == PW && split) ? 1 : 2;   // the wave's private tiles: [pt0, pt1)
  const bool both = wave == PW && nst > PW;
  char* vpriv = vimg + (wave == PW ? PT : PW - 1) * IMG;

  // rows first .. first + n - 1 of a matrix as one 32-row LDS image (rows past n zero)
  auto load_rows = [&](const bf16_t* mat, int ld, size_t first, int n, char* img) {
    const bool ok = r < n;
    const bf16_t* src = mat + (first + (ok ? r : n - 1)) * ld + head * D;
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
      u32x4 x = *reinterpret_cast<const u32x4*>(src + 16 * ks + 8 * h);
      if (!ok) x = u32x4{0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4*>(img + r * (2 * D) + (((2 * ks + h) ^ swz<D>(r)) << 4)) = x;
    }
  };
  const bool shared_on = wave < nst;
  const int sn = slen - 32 * wave < 32 ? slen - 32 * wave : 32;
  if (shared_on) {
    load_rows(p.k, p.ldk, soff + 32 * wave, sn, kimg + wave * IMG);
    load_rows(p.v, p.ldv, soff + 32 * wave, sn, vimg + wave * IMG);
  }

  f32x16 dk[D / 32], dv[D / 32];
#pragma unroll
  for (int dt = 0; dt < D / 32; ++dt) { dk[dt] = f32x16{}; dv[dt] = f32x16{}; }
  const uint32_t halfw = ((uint32_t)p.Tk + 1u) >> 1, halfm = halfw * DROP_M1;
  const float c1 = p.scale * LOG2E;
  const bool dropping = p.drop.thr != 0u;
  const uint32_t thr16 = dropping ? (p.drop.thr >> 16) : 0u;
  const float dsc = dropping ? p.drop.scale : 1.0f;
  int pbuf = 0;

#pragma unroll 1
  for (int m = m0; m < m1; ++m) {
    const int b = sp.g_seq[m];
    if (b < 0 || b >= p.B) continue;
    int ql = p.q_len[b], kl = p.k_len[b];
    ql = ql < 64 ? ql : 64; ql = ql < p.Tq ? ql : p.Tq;
    kl = kl < 0 ? 0 : (kl < 64 ? kl : 64);
    const bool has_s = sp.ks_len[b] > 0 && slen > 0;
    const int Ts = has_s ? slen : 0;
    if (ql <= 0 || kl + Ts <= 0) continue;                       // (workgroup-uniform)
    const int ins = sp.ks_ins < kl ? sp.ks_ins : kl;
    const size_t qbase = (size_t)p.q_off[b], kbase = (size_t)p.k_off[b];
    const int nsh = has_s ? nst : 0;
    const int nqt = (ql + 31) >> 5, npt = (kl + 31) >> 5;        // query tiles, private key tiles
    const bool s_on = wave < nsh, p_on = is_priv && kl > 0;
    pbuf ^= 1;
    char* kpriv = kimg + (PT + 2 * pbuf) * IMG;                  // this sequence's private K images

    // ---- stage the sequence's query tiles
    stage_head<D>(p.q + qbase * p.ldq + head * D, p.ldq, ql, 64, qimg, tid, blockDim.x);
    stage_head<D>(p.dout + qbase * p.lddo + head * D, p.lddo, ql, 64, doimg, tid, blockDim.x);
    {                                                            // delta = rowsum(dO o O): 8 lanes share a row
      const int row = tid >> 3, c = tid & 7;
      float part = 0.f;
      if (row < ql) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(p.dout + (qbase + row) * p.lddo + head * D + 8 * c);
        const u32x4 o = *reinterpret_cast<const u32x4*>(p.o + (qbase + row) * p.ldo + head * D + 8 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          part = fmaf(__uint_as_float(a[e] << 16), __uint_as_float(o[e] << 16), part);
          part = fmaf(__uint_as_float(a[e] & 0xffff0000u), __uint_as_float(o[e] & 0xffff0000u), part);
        }
      }
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) part += __shfl_xor(part, o, 64);
      if (c == 0) del_s[row] = part;
      if (tid < 64) lse_s[tid] = tid < ql ? -p.lse[((size_t)b * p.H + head) * p.Tq + tid] * LOG2E : -INFINITY;
    }
    for (int i = tid; i < NT * 64; i += 512) {                   // mask words of (tile, query), in the tile's key order
      const int t = i >> 6, qi = i & 63;
      const int qc = qi < ql ? qi : ql - 1;
      const uint32_t* mr = p.mask + (size_t)b * p.mask_b_stride + (size_t)qc * p.mask_q_stride;
      uint32_t bits, pad;
      int n;
      if (t < PT) {                                              // shared keys 32 t ..: positions ins + 32 t ..
        bits = mask_bits_at(mr, nw, ins + 32 * t);
        n = Ts - 32 * t;
      } else {                                                   // private key i: position i below ins, else i + Ts
        const int k0 = 32 * (t - PT), c = ins - k0;              // c: keys of this tile ahead of the segment
        const uint32_t lo = mask_bits_at(mr, nw, k0), hi = mask_bits_at(mr, nw, k0 + Ts);
        bits = c >= 32 ? lo : (c <= 0 ? hi : ((lo & ((1u << c) - 1u)) | (hi & ~((1u << c) - 1u))));
        n = kl - k0;
      }
      pad = n >= 32 ? 0u : (n <= 0 ? ~0u : ~0u << n);
      mw_s[i] = ~bits | pad;
    }
    if (p_on)
      for (int pt = pt0; pt < pt1 && pt < npt; ++pt)
        load_rows(p.k, p.ldk, kbase + 32 * pt, kl - 32 * pt < 32 ? kl - 32 * pt : 32, kpriv + pt * IMG);
    stage_wait();
    __syncthreads();

    // S, dP, P, dS of key tile t (its key on the lane, at position kpos; K / V images kt / vt) against query tile qt
    auto tile_pass = [&](int t, int qt, const char* kt, const char* vt, int kpos) {
      const char* qi = qimg + qt * IMG;
      const char* di = doimg + qt * IMG;
      char* ws = scr + (t * 2 + qt) * 2048;
      const uint32_t lin0 = drop_lin(p.drop, (((uint32_t)b * p.H + head) * (uint32_t)p.Tq + 32u * (uint32_t)qt) * halfw + ((uint32_t)kpos >> 1));
      f32x16 sacc = {}, dpacc = {};
#pragma unroll
      for (int ks = 0; ks < D / 16; ++ks) {
        const bf16x8 qf = read_row_frag<D>(qi, r, 2 * ks + h);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, read_row_frag<D>(kt, r, 2 * ks + h), sacc, 0, 0, 0);
        const bf16x8 df = read_row_frag<D>(di, r, 2 * ks + h);
        dpacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(df, read_row_frag<D>(vt, r, 2 * ks + h), dpacc, 0, 0, 0);
      }
      float pd[16], ds[16];
      spl_score_tile(p.drop, lin0, halfm, ((uint32_t)kpos & 1u) << 4, thr16, dsc, c1, dropping, sacc, dpacc, lse_s + 32 * qt, del_s + 32 * qt,
                     mw_s + t * 64 + 32 * qt, r, h, pd, ds);
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        *reinterpret_cast<u32x2*>(ws + r * 64 + (((2 * g4 + h) ^ tile64_swz(r)) << 3)) =
            u32x2{pack2bf(ds[4 * g4], ds[4 * g4 + 1]), pack2bf(ds[4 * g4 + 2], ds[4 * g4 + 3])};
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        const bf16x8 pf = pack8(pd + 8 * ss);
        const bf16x8 dsf = pack8(ds + 8 * ss);
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) {
          const bf16x8 dotf = read_tr_frag<D>(di, 16 * ss, 32 * dt, lane);
          dv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dotf, pf, dv[dt], 0, 0, 0);
          const bf16x8 qtf = read_tr_frag<D>(qi, 16 * ss, 32 * dt, lane);
          dk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qtf, dsf, dk[dt], 0, 0, 0);
        }
      }
    };
#pragma unroll 1
    for (int job = 0; job < 3; ++job) {                          // the wave's shared tile, private tile 0, private tile 1: one copy of the code
      const bool priv = job > 0;
      const int pt = job - 1;
      if (priv ? !(p_on && pt >= pt0 && pt < pt1 && pt < npt) : !s_on) continue;          // (wave-uniform: the lane swap of the stores needs every lane)
      const int pn = kl - 32 * pt < 32 ? kl - 32 * pt : 32;      // (private) keys of the tile
      if (priv) {
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            if (both && pt == pt0) { park[(32 * dt + e) * 64 + lane] = dk[dt][e]; park[(32 * dt + 16 + e) * 64 + lane] = dv[dt][e]; }
            dk[dt][e] = 0.f; dv[dt][e] = 0.f;
          }
      }
      if (priv) load_rows(p.v, p.ldv, kbase + 32 * pt, pn, vpriv);
      const int ki = 32 * pt + r;                                // (private) the lane's key
      const int t = priv ? PT + pt : wave;
      const char* kt = priv ? kpriv + pt * IMG : kimg + wave * IMG;
      const int kpos = priv ? (ki < ins ? ki : ki + Ts) : ins + 32 * wave + r;
#pragma unroll 1
      for (int qt = 0; qt < nqt; ++qt) tile_pass(t, qt, kt, priv ? vpriv : vimg + wave * IMG, kpos);
      if (priv) {
        const bool ok = r < pn;
        store_acc_row<D>(p.dk + (kbase + (ok ? ki : 0)) * p.lddk + head * D, dk, p.scale, h, ok);
        store_acc_row<D>(p.dv + (kbase + (ok ? ki : 0)) * p.lddv + head * D, dv, 1.0f, h, ok);
        if (both && (pt == npt - 1 || pt == pt1 - 1)) {
#pragma unroll
          for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) { dk[dt][e] = park[(32 * dt + e) * 64 + lane]; dv[dt][e] = park[(32 * dt + 16 + e) * 64 + lane]; }
        }
      }
    }
    __syncthreads();                                             // every tile's dS^T is in LDS
    // ---- dQ^T, output-stationary: wave 3 + 2 qt + dt owns the 32-wide slice dt of D of query tile qt over every key tile, in
    // tile order.  The other waves go on to stage the next sequence: nothing read here is rewritten before the next staging
    // barrier, the private K images alternate.
    if (wave >= 3 && wave <= 6) {
      const int qt = (wave - 3) >> 1, dt = (wave - 3) & 1;
      if (qt < nqt) {
        f32x16 dq1[1] = {f32x16{}};
        const int ntile = nsh + npt;
        for (int i = 0; i < ntile; ++i) {
          const int t = i < nsh ? i : PT + (i - nsh);
          const char* ki = t < PT ? kimg + t * IMG : kpriv + (t - PT) * IMG;
#pragma unroll
          for (int ss = 0; ss < 2; ++ss) {
            const bf16x8 ktf = read_tr_frag<D>(ki, 16 * ss, 32 * dt, lane);
            const bf16x8 dstf = read_tr_tile64s(scr + (t * 2 + qt) * 2048, 16 * ss, lane);
            dq1[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf, dstf, dq1[0], 0, 0, 0);
          }
        }
        const int qr = 32 * qt + r;
        const bool ok = qr < ql;
        store_acc_row<32>(p.dq + (qbase + (ok ? qr : 0)) * p.lddq + head * D + 32 * dt, dq1, p.scale, h, ok);
      }
    }
  }

  if (shared_on) {                                               // the segment's rows: one rounding of the fp32 sums
    const bool ok = r < sn;
    bf16_t* dkg = p.dk + (soff + 32 * wave + (ok ? r : 0)) * p.lddk + head * D;
    bf16_t* dvg = p.dv + (soff + 32 * wave + (ok ? r : 0)) * p.lddv + head * D;
    if (!sp.accumulate) {
      store_acc_row<D>(dkg, dk, p.scale, h, ok);
      store_acc_row<D>(dvg, dv, 1.0f, h, ok);
    } else if (ok) {                                             // ... together with what the rows hold
#pragma unroll
      for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
          const int d0 = 32 * dt + 8 * gg + 4 * h;               // registers 4 gg .. 4 gg + 3 = columns d0 .. d0 + 3
          u32x2* pk = reinterpret_cast<u32x2*>(dkg + d0);
          u32x2* pv = reinterpret_cast<u32x2*>(dvg + d0);
          const u32x2 hk = *pk, hv = *pv;
          *pk = u32x2{pack2bf(fmaf(dk[dt][4 * gg], p.scale, __uint_as_float(hk[0] << 16)),
                              fmaf(dk[dt][4 * gg + 1], p.scale, __uint_as_float(hk[0] & 0xffff0000u))),
                      pack2bf(fmaf(dk[dt][4 * gg + 2], p.scale, __uint_as_float(hk[1] << 16)),
                              fmaf(dk[dt][4 * gg + 3], p.scale, __uint_as_float(hk[1] & 0xffff0000u)))};
          *pv = u32x2{pack2bf(dv[dt][4 * gg] + __uint_as_float(hv[0] << 16), dv[dt][4 * gg + 1] + __uint_as_float(hv[0] & 0xffff0000u)),
                      pack2bf(dv[dt][4 * gg + 2] + __uint_as_float(hv[1] << 16), dv[dt][4 * gg + 3] + __uint_as_float(hv[1] & 0xffff0000u))};
        }
    }
  }
}

// ---- launches.  A workgroup is one (sequence, head) item: `parts` = 1, written by the fill functions below.  (Two 4-wave workgroups
// per item fit two to a CU and overlap each other's staging, but both stage the full images: 589 vs 545 us for the text fwd+bwd trio.)
//
// Threads per workgroup: one wave per 32-row tile that computes, but never fewer than the staging needs.
// The co-attention direction with 37 region queries (or keys) has 2 compute waves and 2 x 64 KiB of text
// K/V (or Q/dO) to stage; with 128 threads that is 32 dependent load->ds_write rounds per image.  Extra
// waves stage, then leave at the per-wave exit right after the barrier.
inline int block_threads(int tiles, int staged_rows) {
  return (staged_rows >= 128 && tiles < 8 ? 8 : tiles) * 64;
}

template <typename K>
int set_lds(K kern, size_t lds) {
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return UNIMM_E_HIP;
  return UNIMM_OK;
}

// One launch of `grid` workgroups: lds_bytes is the kernel's layout (L::bytes), and nothing else
template <typename K, typename P>
int launch_items(K kern, size_t lds_bytes, int grid, int threads, const P& params, hipStream_t s) {
  if (set_lds(kern, lds_bytes) != UNIMM_OK) return UNIMM_E_HIP;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds_bytes, s, params);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

template <int D, int NKT>
int launch_bwd_dq(const AttnBwdParams& p, hipStream_t s) {
  const int tiles = (p.Tq + 31) / 32;
  return launch_items(attn_bwd_dq_kernel<D, NKT>, KvImagesLds<D, NKT>::bytes, p.B * p.H, block_threads(tiles, NKT * 32), p, s);
}

template <int D, int NQT>
int launch_bwd_dkv(const AttnBwdParams& p, hipStream_t s) {
  const int tiles = (p.Tk + 31) / 32;
  if constexpr (D == 128 && NQT == 8) {   // (the 37x37 image self-attention, NQT = 2, lives on many small workgroups per CU)
    if (tiles <= 2) return launch_items(attn_bwd_dkv_kernel<D, NQT, 256>, BwdDkvLds<D, NQT>::bytes, p.B * p.H, 256, p, s);
  }
  return launch_items(attn_bwd_dkv_kernel<D, NQT>, BwdDkvLds<D, NQT>::bytes, p.B * p.H, block_threads(tiles, NQT * 32), p, s);
}

template <int D, int NKT>
int launch_fwd(const AttnParams& p, hipStream_t s) {
  int threads = block_threads((p.Tq + 31) / 32, NKT * 32);
  if (D == 64 && threads > 256) threads = 256;   // 4 waves walk the 8 query tiles: two workgroups per CU
  return launch_items(attn_fwd_kernel<D, NKT>, KvImagesLds<D, NKT>::bytes, p.B * p.H, threads, p, s);
}

// ------------------------------------------------------------------------------------------------
// attention probabilities as a tensor (models/vilbert_dialog.py:401-405 returns them; the encoder collects them when
// output_all_attention_masks is set, :855-929).  Not on the hot path: the fused kernels above never materialise P.
// One wave per (sequence, head, query) row of the fixed layout; a lane owns keys lane, lane + 64, ...; fp32
// softmax(q . k * scale + additive mask) from the bf16 operands, then the SAME dropout words as attn_fwd.
// ------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void attn_probs_kernel(AttnParams p, float* __restrict__ probs) {
  drop_resolve(p.drop);
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);           // (b * H + head) * Tq + q
  const long nrows = (long)p.B * p.H * p.Tq;
  if (row >= nrows) return;
  const int q = (int)(row % p.Tq);
  const int bh = (int)(row / p.Tq), head = bh % p.H, b = bh / p.H;
  const bf16_t* qg = p.q + ((size_t)b * p.Tq + q) * p.ldq + head * D;
  float qv[D];
#pragma unroll
  for (int c = 0; c < D / 8; ++c) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(qg + 8 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e) { qv[8 * c + 2 * e] = __uint_as_float(v[e] << 16); qv[8 * c + 2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u); }
  }
  const uint32_t* mrow = p.mask + (size_t)b * p.mask_b_stride + (size_t)q * p.mask_q_stride;
  float sc[4];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key = lane + 64 * j;
    sc[j] = -INFINITY;
    if (key < p.Tk) {
      const bf16_t* kg = p.k + ((size_t)b * p.Tk + key) * p.ldk + head * D;
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < D / 8; ++c) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(kg + 8 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc = fmaf(qv[8 * c + 2 * e], __uint_as_float(v[e] << 16), acc);
          acc = fmaf(qv[8 * c + 2 * e + 1], __uint_as_float(v[e] & 0xffff0000u), acc);
        }
      }
      const bool ok = (mrow[key >> 5] >> (key & 31)) & 1u;
      sc[j] = acc * p.scale + (ok ? 0.f : -10000.0f);
      mx = fmaxf(mx, sc[j]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sc[j] = (lane + 64 * j) < p.Tk ? __expf(sc[j] - mx) : 0.f;
    sum += sc[j];
  }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  float* out = probs + (size_t)row * p.Tk;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key = lane + 64 * j;
    if (key >= p.Tk) continue;
    float v = sc[j] * inv;
    if (p.drop.thr != 0u) v = drop_apply(p.drop, (uint32_t)row, (uint32_t)p.Tk, (uint32_t)key, v);
    out[key] = v;
  }
}

// ---- arguments -> kernel parameters, one function per argument family.  The order of the checks is part of the interface
// (tests/test_attention_refusals.py): pointers (UNIMM_E_ARG), shape, alignment, then the words that describe the layout.
// unimm_attn_args.  values = false: a launch that reads q, k and the mask only (v, out and their strides are not looked at).
int fill_fwd(const unimm_attn_args* a, AttnParams& p, bool values) {
  if (a == nullptr || !a->q || !a->k || !a->mask || (values && (!a->v || !a->out))) return UNIMM_E_ARG;
  if (a->B <= 0 || a->H <= 0 || a->Tq <= 0 || a->Tk <= 0 || a->Tq > 256 || a->Tk > 256) return UNIMM_E_SHAPE;
  if (a->D != 64 && a->D != 128) return UNIMM_E_SHAPE;
  if ((a->ldq % 8) || (a->ldk % 8) || (values && ((a->ldv % 8) || (a->ldo % 8)))) return UNIMM_E_ALIGN;   // result rows leave as 16-byte stores (store_acc_row)
  if (((uintptr_t)a->q | (uintptr_t)a->k) & 15) return UNIMM_E_ALIGN;
  if (values && (((uintptr_t)a->v | (uintptr_t)a->out) & 15)) return UNIMM_E_ALIGN;
  if ((a->q_off == nullptr) != (a->q_len == nullptr) || (a->k_off == nullptr) != (a->k_len == nullptr)) return UNIMM_E_ARG;
  if ((a->ks_off == nullptr) != (a->ks_len == nullptr)) return UNIMM_E_ARG;
  if (a->ks_off != nullptr && (a->k_off == nullptr || a->ks_ins < 0)) return UNIMM_E_ARG;   // a shared segment: variable-length keys
  p.q = (const bf16_t*)a->q; p.k = (const bf16_t*)a->k; p.v = (const bf16_t*)a->v;
  p.o = (bf16_t*)a->out; p.lse = a->lse; p.mask = a->mask;
  p.q_off = a->q_off; p.q_len = a->q_len; p.k_off = a->k_off; p.k_len = a->k_len;
  p.ks_off = a->ks_off; p.ks_len = a->ks_len; p.ks_ins = a->ks_off != nullptr ? a->ks_ins : 0;
  p.order = a->order;
  p.B = a->B; p.H = a->H; p.Tq = a->Tq; p.Tk = a->Tk;
  p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo;
  p.mask_q_stride = a->mask_q_stride; p.mask_b_stride = a->mask_b_stride;
  p.parts = 1;
  p.scale = a->scale;
  p.drop.key = a->drop_key; p.drop.thr = a->drop_thr; p.drop.scale = a->drop_scale; p.drop.salt = a->drop_salt; p.drop.key2 = 0u;
  return UNIMM_OK;
}

// unimm_attn_bwd_args and unimm_attn_spliced_bwd_args (the same fields, then the segment and the groups).  `delta` is the caller's
// to require; bad_shape: what a shape that no kernel takes is called (the spliced entries take one shape: UNIMM_E_ARG).
template <typename A>
int fill_bwd(const A* a, AttnBwdParams& p, int bad_shape) {
  if (a == nullptr || !a->q || !a->k || !a->v || !a->out || !a->dout || !a->lse || !a->dq || !a->dk || !a->dv || !a->mask)
    return UNIMM_E_ARG;
  if (a->B <= 0 || a->H <= 0 || a->Tq <= 0 || a->Tk <= 0 || a->Tq > 256 || a->Tk > 256) return bad_shape;
  if (a->D != 64 && a->D != 128) return bad_shape;
  if ((a->ldq % 8) || (a->ldk % 8) || (a->ldv % 8) || (a->ldo % 8) || (a->lddo % 8) || (a->lddq % 8) || (a->lddk % 8) ||
      (a->lddv % 8))
    return UNIMM_E_ALIGN;                                         // dQ / dK / dV rows leave as 16-byte stores (store_acc_row)
  if (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->out | (uintptr_t)a->dout | (uintptr_t)a->dq |
       (uintptr_t)a->dk | (uintptr_t)a->dv) & 15)
    return UNIMM_E_ALIGN;
  p.q = (const bf16_t*)a->q; p.k = (const bf16_t*)a->k; p.v = (const bf16_t*)a->v; p.o = (const bf16_t*)a->out;
  p.dout = (const bf16_t*)a->dout; p.lse = a->lse; p.delta = a->delta;
  p.dq = (bf16_t*)a->dq; p.dk = (bf16_t*)a->dk; p.dv = (bf16_t*)a->dv; p.mask = a->mask;
  p.q_off = a->q_off; p.q_len = a->q_len; p.k_off = a->k_off; p.k_len = a->k_len;
  p.order = a->order;
  p.B = a->B; p.H = a->H; p.Tq = a->Tq; p.Tk = a->Tk;
  p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo; p.lddo = a->lddo;
  p.lddq = a->lddq; p.lddk = a->lddk; p.lddv = a->lddv;
  p.mask_q_stride = a->mask_q_stride; p.mask_b_stride = a->mask_b_stride;
  p.parts = 1;
  p.scale = a->scale;
  p.drop.key = a->drop_key; p.drop.thr = a->drop_thr; p.drop.scale = a->drop_scale; p.drop.salt = a->drop_salt; p.drop.key2 = 0u;
  return UNIMM_OK;
}

}  // namespace

// unimm_attn_fwd, and (train_seg) unimm_attn_spliced_fwd: the same launch with dropout allowed beside a shared segment
static int attn_fwd_entry(const unimm_attn_args* a, void* stream, bool train_seg) {
  AttnParams p;
  const int rc = fill_fwd(a, p, true);
  if (rc != UNIMM_OK) return rc;
  if (p.ks_off != nullptr && a->drop_thr != 0u && !train_seg) return UNIMM_E_ARG;   // a shared segment through unimm_attn_fwd: inference
  hipStream_t s = (hipStream_t)stream;
  const int items = p.B * p.H;
  const bool small_k = a->Tk <= 64;
  if (a->D == 64) return small_k ? launch_fwd<64, 2>(p, s) : launch_fwd<64, 8>(p, s);
  if (UNIMM_ATTN_FEWQ_FWD && !small_k && a->Tq <= 64 && p.ks_off == nullptr)      // few queries, many keys
    return launch_items(attn_fwd_fewq128_kernel, FwdFewq128Lds::bytes, items, 512, p, s);
  return small_k ? launch_fwd<128, 2>(p, s) : launch_fwd<128, 8>(p, s);
}

extern "C" int unimm_attn_fwd(const unimm_attn_args* a, void* stream) { return attn_fwd_entry(a, stream, false); }

static int attn_spliced_fwd_entry(const unimm_attn_args* a, void* stream, int max_tq) {
  if (a == nullptr || !a->q || !a->k || !a->v || !a->out || !a->mask || !a->lse) return UNIMM_E_ARG;
  if (!a->q_off || !a->q_len || !a->k_off || !a->k_len || !a->ks_off || !a->ks_len || a->ks_ins < 0) return UNIMM_E_ARG;
  if (a->B <= 0 || a->H <= 0 || a->D != 64 || a->Tq <= 0 || a->Tq > max_tq || a->Tk <= 0 || a->Tk > 256) return UNIMM_E_ARG;
  return attn_fwd_entry(a, stream, true);
}
extern "C" int unimm_attn_spliced_fwd(const unimm_attn_args* a, void* stream) { return attn_spliced_fwd_entry(a, stream, 32); }
extern "C" int unimm_attn_spliced_wide_fwd(const unimm_attn_args* a, void* stream) { return attn_spliced_fwd_entry(a, stream, 64); }

extern "C" int unimm_attn_probs(const unimm_attn_args* a, float* probs, void* stream) {
  if (a == nullptr || !probs) return UNIMM_E_ARG;
  if (a->q_off || a->q_len || a->k_off || a->k_len || a->ks_off || a->ks_len) return UNIMM_E_ARG;   // fixed layout only
  AttnParams p;
  const int rc = fill_fwd(a, p, false);
  if (rc != UNIMM_OK) return rc;
  const long rows = (long)a->B * a->H * a->Tq;
  const unsigned blocks = (unsigned)((rows + 3) / 4);
  if (a->D == 64) hipLaunchKernelGGL(attn_probs_kernel<64>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, probs);
  else hipLaunchKernelGGL(attn_probs_kernel<128>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, probs);
  UNIMM_CHECK_LAUNCH();
  return UNIMM_OK;
}

extern "C" int unimm_attn_bwd(const unimm_attn_bwd_args* a, void* stream) {
  if (a == nullptr || !a->delta) return UNIMM_E_ARG;
  AttnBwdParams p;
  int rc = fill_bwd(a, p, UNIMM_E_SHAPE);
  if (rc != UNIMM_OK) return rc;
  if ((p.q_off == nullptr) != (p.q_len == nullptr) || (p.k_off == nullptr) != (p.k_len == nullptr)) return UNIMM_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int items = p.B * p.H;
  const bool small_k = a->Tk <= 64, small_q = a->Tq <= 64;
  if (a->D == 64 && !small_k && !small_q)                         // text self-attention: one kernel
    return launch_items(attn_bwd_fused_kernel<8>, BwdFusedLds<8>::bytes, items, 512, p, s);
  // regions attend text (37 queries x up to 256 keys): one kernel, 133 against 94 + 134 us per layer at 240 sequences.  (The 37 x 37
  // image self-attention stays on the pair of small workgroups: two active key-tile waves in a one-per-CU workgroup were 95 against 81 us.)
  if (UNIMM_ATTN_FEWQ128 && a->D == 128 && small_q && !small_k)
    return launch_items(attn_bwd_fewq128_kernel<2>, BwdFewq128Lds<2>::bytes, items, 512, p, s);
  if (UNIMM_ATTN_FEWK128 && a->D == 128 && small_k && !small_q)   // text attends regions: one kernel
    return launch_items(attn_bwd_fewk128_kernel, BwdFewk128Lds::bytes, items, 512, p, s);
  if (a->D == 64) rc = small_k ? launch_bwd_dq<64, 2>(p, s) : launch_bwd_dq<64, 8>(p, s);
  else rc = small_k ? launch_bwd_dq<128, 2>(p, s) : launch_bwd_dq<128, 8>(p, s);
  if (rc != UNIMM_OK) return rc;
  if (a->D == 64) return small_q ? launch_bwd_dkv<64, 2>(p, s) : launch_bwd_dkv<64, 8>(p, s);
  return small_q ? launch_bwd_dkv<128, 2>(p, s) : launch_bwd_dkv<128, 8>(p, s);
}

// unimm_attn_spliced_bwd (max_tq = 32) and unimm_attn_spliced_wide_bwd (max_tq = 64): the same checks and arguments, their own kernels
static int attn_spliced_bwd_entry(const unimm_attn_spliced_bwd_args* a, void* stream, int max_tq) {
  if (a == nullptr) return UNIMM_E_ARG;
  if (!a->q_off || !a->q_len || !a->k_off || !a->k_len || !a->ks_off || !a->ks_len || a->ks_ins < 0) return UNIMM_E_ARG;
  if (!a->g_first || !a->g_seq || a->G <= 0) return UNIMM_E_ARG;
  if (a->D != 64 || a->Tq > max_tq) return UNIMM_E_ARG;           // (the other bounds: fill_bwd)
  AttnSplBwdParams sp;
  const int rc = fill_bwd(a, sp.b, UNIMM_E_ARG);
  if (rc != UNIMM_OK) return rc;
  sp.b.delta = nullptr; sp.b.order = nullptr;                     // not read: a workgroup is a (group, head), delta is formed in the kernel
  sp.ks_off = a->ks_off; sp.ks_len = a->ks_len; sp.ks_ins = a->ks_ins;
  sp.g_first = a->g_first; sp.g_seq = a->g_seq; sp.G = a->G;
  sp.accumulate = a->accumulate;
  hipStream_t s = (hipStream_t)stream;
  if (max_tq > 32) return launch_items(attn_spliced_wide_bwd_kernel, SplicedBwdLds<2>::bytes, a->G * a->H, 512, sp, s);
  return launch_items(attn_spliced_bwd_kernel, SplicedBwdLds<1>::bytes, a->G * a->H, 512, sp, s);
}

extern "C" int unimm_attn_spliced_bwd(const unimm_attn_spliced_bwd_args* a, void* stream) { return attn_spliced_bwd_entry(a, stream, 32); }
extern "C" int unimm_attn_spliced_wide_bwd(const unimm_attn_spliced_bwd_args* a, void* stream) { return attn_spliced_bwd_entry(a, stream, 64); }
