/* unimm_hip.h -- C ABI of libunimm_hip.so: hand-written gfx950 (MI355X) kernels for the UniMM-UL
 * forward/backward hot path.
 *
 * The reference (ZihaoW123/UniMM) is pure Python/PyTorch and has no FFI of its own (SURVEY.md 2:
 * no .cu/.cpp, no custom op).  The "interface each entry point replaces" is therefore a torch-op
 * chain inside models/vilbert_dialog.py; every declaration below cites it (file:line relative to
 * the reference root).  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions: extern "C"; every pointer is a DEVICE pointer on the current HIP device; `stream`
 * is a hipStream_t passed as void*; bf16 tensors are uint16 bit patterns; row strides ("ld") are in
 * elements.  Calls only enqueue work (no allocation, no synchronisation) and return UNIMM_OK or a
 * negative UNIMM_E_* code; they never throw.
 */
#ifndef UNIMM_HIP_H
#define UNIMM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNIMM_OK 0
#define UNIMM_E_ARG (-1)   /* null pointer / unknown enum value */
#define UNIMM_E_SHAPE (-2) /* unsupported size */
#define UNIMM_E_ALIGN (-3) /* pointer or stride alignment */
#define UNIMM_E_HIP (-4)   /* launch failed */

int unimm_version(void);          /* ABI version, bumped on any signature change */
const char* unimm_arch(void);     /* "gfx950" */

/* ---------------------------------------------------------------------------------------------
 * GEMM, "NT": OUT[M,N] = epilogue( X[M,K] . W[N,K]^T ), bf16 operands, fp32 accumulate.
 * Replaces every nn.Linear forward on the path (models/vilbert_dialog.py:386-388, 423, 453, 466,
 * 515-517, 552, 582, 595, 659-661, 670-672, 745-748, 950, 965, 983, 1002, 1025, 1070, 1087,
 * 1488-1489) with the elementwise op that follows it fused in, and -- called with the transposed
 * bf16 weight copy -- the input-gradient half of their autograd backward.
 * K % 64 == 0; ldx, ldw % 8 == 0; ldo, ldaux % 4 == 0; x, w, out and -- where given -- aux and out2 16-byte aligned
 * (UNIMM_E_ALIGN otherwise: the epilogue reads aux and writes out2 sixteen bytes at a time wherever the row stride keeps rows
 * aligned; every caller in this repository passes whole allocations or row slices of them).  bias and the aux_* vectors are
 * read one fp32 at a time and need only their natural 4-byte alignment.
 * ------------------------------------------------------------------------------------------- */
enum {
  UNIMM_EPI_BIAS = 0,            /* out = acc + bias                                            */
  UNIMM_EPI_BIAS_GELU = 1,       /* u = acc + bias; out = erf-GELU(u) (:115-121); out2 = u      */
  UNIMM_EPI_BIAS_DROP_RESID = 2, /* out(fp32) = dropout(acc + bias) + aux(fp32 residual stream) (:423-425, :466-468, ...) */
  UNIMM_EPI_BIAS_RELU = 3,       /* poolers (:950-951, :965-966)                                */
  UNIMM_EPI_DGELU = 4,           /* out = acc * GELU'(aux)           (backward of :453-454)     */
  UNIMM_EPI_ADD = 5,             /* out = acc + aux                  (residual gradient join)   */
  UNIMM_EPI_MUL = 6,             /* out = acc * aux                  (backward of GELU with aux = GELU'(u)) */
  UNIMM_EPI_BIAS_GELU_DG = 7     /* u = acc + bias; out = erf-GELU(u); out2 = GELU'(u) (training FFN) */
};

typedef struct {
  const void* x;     /* [M, K] bf16 */
  const void* w;     /* [N, K] bf16 */
  const float* bias; /* [N] fp32 or NULL */
  const void* aux;   /* [M, N] epilogue operand or NULL: fp32 residual (DROP_RESID), bf16 otherwise */
  void* out;         /* [M, N] bf16, or fp32 when out_f32 != 0 */
  void* out2;        /* [M, N] bf16 second output of UNIMM_EPI_BIAS_GELU (row stride ldo) or NULL */
  int32_t M, N, K;
  int32_t ldx, ldw, ldaux, ldo;
  int32_t epilogue;
  int32_t out_f32;
  uint32_t drop_key; /* dropout (UNIMM_EPI_BIAS_DROP_RESID): element (m, n) is kept iff the 16-bit field (n & 1) of
                      * drop_word(key, m * ceil(N / 2) + n / 2) is >= thr -- one counter-based hash per two neighbouring
                      * columns (csrc/common.h: drop_word; unimm_amd/dropout.py is the bit-exact host mirror)  */
  uint32_t drop_thr; /* p * 2^32 (dropout.py: drop_arg); the kernels compare each 16-bit field with thr >> 16, so p is
                      * resolved to 2^-16; 0 disables                                           */
  float drop_scale;  /* 1 / (1 - p)                                                             */
  /* UNIMM_EPI_BIAS_DROP_RESID only, all four or none: the residual operand is LayerNorm(aux) evaluated on
   * the fly, (aux[m,n] - aux_mean[m]) * aux_rstd[m] * aux_gamma[n] + aux_beta[n] -- the fp32 output of the
   * previous LayerNorm (models/vilbert_dialog.py:425, :468, ...) is then never written or read */
  const float* aux_mean;
  const float* aux_rstd;
  const float* aux_gamma;
  const float* aux_beta;
  /* Per-call tuning (tests and A/B measurements; 0 = everything automatic): tile = gn * 1000 + p * 100 + cfg.
   *   cfg: 0 automatic (a cost model over {256x256, 192x256, 128x128}; 64x128 for grids that do not fill the chip),
   *        1 = 128x128 / 4 waves / 2-slot ring of BK 64 / 2 workgroups per CU,   3 = 256x256 / 8 waves / lock-step ring,
   *        6 = 192x256 / 8 waves,   7 = 64x128 / 4 waves of 32x64 / 3 workgroups per CU,   8 = 256x256 / ping-pong loop,
   *        9 = 64x128 with a 3-slot ring (two K steps in flight, 2 workgroups per CU),   10 = 128x128 with a 3-slot ring (1 per CU),
   *        12 / 14 / 15 = 192x256 / 128x128 / 64x128 with the X operand alone on a three-slot ring (W stays on two: X(t+2) is in
   *        flight while step t computes -- in a training step X was just written by the previous kernel and streams from HBM;
   *        12 is what the automatic choice uses for its 192x256 class);  anything else is rejected with UNIMM_E_ARG
   *   p:   0 automatic, 1 persistent workgroups (one per CU slot walks several tiles), 2 one workgroup per tile
   *   gn:  n-tiles per column group of the tile order (0 = default 4) */
  int32_t tile;
  /* or NULL: a device word XORed into drop_key at kernel entry.  The argument then carries the per-(seed, site) part of the
   * key and memory the per-step part, so that a captured / replayed launch (unimm_amd/graphs.py) draws a fresh mask every
   * step; unimm_amd/dropout.py: make_key(seed, step, site) = site_key(seed, site) ^ step_salt(seed, step).  Every entry
   * point that takes a dropout triple takes such a word. */
  const uint32_t* drop_salt;
  /* Split-K for grids that leave the chip under-filled (the ~4-8k rows of a 30-60-sequence share of a split batch against
   * K = 2304 / 3072: a few hundred tiles, each a 36-48 step dependent chain).  splitk: 0 / 1 = off; 2 .. 8 = at most that many
   * workgroups per output tile, each reducing a slice of K; -1 = the library's choice (as many as stay resident at once, <= 4,
   * >= 8 K-steps each).  Partial tiles meet in the caller's workspace and the last arriver of a tile runs the epilogue, so the
   * fused epilogues work unchanged.  splitk_ws: 256-byte aligned device memory, ZERO-FILLED ONCE by the caller and then private
   * to launches of ONE stream (the kernel leaves its counters zero); 16 KiB of counters (one int32 ticket per output tile, so at
   * most 4096 tiles) + tiles * splits * tile bytes, a tile being BM x BN fp32 partial sums (a 64 x 128 tile is 32 KiB, 128 x 128
   * 64 KiB), `splits` the number the launch settles on; too small for that = the launch runs unsplit (not with fewer splits).
   * A split request (splitk other than 0 / 1) with no workspace or fewer than 32 KiB of it is rejected with UNIMM_E_ARG.
   * Four-wave ring-loop tiles only (64x128: 7, 9, 15; 128x128: 1, 10, 14); on every other tile the request is ignored.
   * oracle/gemm_ref.py (splits, ws_bytes) restates these rules for the tests. */
  void* splitk_ws;
  int64_t splitk_ws_bytes;
  int32_t splitk;
  /* UNIMM_EPI_BIAS_DROP_RESID on a SUBSET of rows (each int32 [M] or NULL = the identity; UNIMM_E_ARG with another epilogue).
   * drop_rows: output row m draws the dropout mask of row drop_rows[m], i.e. the mask the same launch over all rows gives
   * that row.  aux_rows: the residual operand and, where given, its LayerNorm statistics (aux, aux_mean, aux_rstd) are read
   * at row aux_rows[m] -- the rows of a gathered block read their residual straight from the full-row stream.  Every entry
   * must name a valid row, those of surplus (capacity) rows included; an entry may repeat. */
  const int32_t* drop_rows;
  const int32_t* aux_rows;
} unimm_gemm_nt_args;

int unimm_gemm_nt(const unimm_gemm_nt_args* args, void* stream);

/* GEMM, "TN": DW[N,K] += DY[M,N]^T . X[M,K] (fp32 atomics; caller zeroes DW once per step) and,
 * when dbias != NULL, dbias[N] += column sums of DY (the bias gradient, one extra MFMA per tile).
 * Weight-gradient half of every nn.Linear backward on the path.  Rows of DY / X must be readable
 * up to round_up(N, 8) / round_up(K, 8) columns; lddy, ldx % 8 == 0. */
typedef struct {
  const void* dy; /* [M, N] bf16 */
  const void* x;  /* [M, K] bf16 */
  float* dw;      /* [N, K] fp32, row stride lddw */
  float* dbias;   /* [N] fp32 or NULL */
  int32_t M, N, K;
  int32_t lddy, ldx, lddw;
  const int32_t* m_dev; /* or NULL: device word holding the number of reduction rows actually present; M is then the
                         * CAPACITY the launch is sized for (replayed launch sequences: see unimm_plan_build) */
  int32_t overwrite;    /* != 0: DW = DY^T X instead of +=.  The caller asserts that dw is all zero and that no other problem,
                         * launch or stream adds to it concurrently; a tile reduced by one workgroup is then written with plain
                         * stores (no memory-side atomics).  Ignored (+= as usual) where the reduction is split.  dbias always +=.
                         * ABI 16. */
} unimm_gemm_tn_args;

int unimm_gemm_tn(const unimm_gemm_tn_args* args, void* stream);
/* `count` independent TN problems (host array) in as few grids as possible: the weight gradients of one
 * encoder block (models/vilbert_dialog.py:386-388, 423-425, 453-454, 466-468 and twins) in one launch.
 * Same result as `count` calls of unimm_gemm_tn; the problems may alias each other's dw / dbias when they are
 * meant to accumulate (every path, with or without a workspace, ends in fp32 atomics). */
int unimm_gemm_tn_grouped(const unimm_gemm_tn_args* args, int32_t count, void* stream);
/* The same with (a) the "launches share the chip with another stream's kernels" hint of the split heuristic
 * (shared_chip != 0: fewer, longer workgroups and fewer partial tiles), and (b) a caller-owned WORKSPACE: when the
 * reduction is split, every split stores its fp32 partial tile to a slab of the workspace (plain coalesced stores) and
 * the split that arrives last at the tile's counter sums the slabs and adds the tile into dw once, instead of every
 * split adding 256 KiB with memory-side atomics (8x the algorithmic write traffic, a ~43 us drain per launch).
 * ws: 256-byte aligned device memory, ZERO-FILLED ONCE by the caller before its first use and then private to launches
 * of ONE stream (the kernels leave the counters zero); ws_bytes >= 16 KiB + tiles * splits * tile bytes
 * (512 MiB covers every launch of the full config at 240 sequences); too small or NULL = the atomic path.
 * The result equals the atomic path's up to the order of the fp32 sums (the last arriver adds the other splits'
 * partials to its own in index order). */
int unimm_gemm_tn_grouped_ws(const unimm_gemm_tn_args* args, int32_t count, int32_t shared_chip, void* ws, int64_t ws_bytes,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused attention core: out = dropout(softmax(Q K^T * scale + additive(mask))) V per (sequence,
 * head); additive(mask) = (1 - bit) * -10000 exactly as models/vilbert_dialog.py:1415-1431.
 * Replaces :390-410 (text, Tq=Tk=256, D=64, dense mask), :519-539 (image, 37x37, D=128, key mask)
 * and both directions of :681-721 (256x37 with the image key mask; 37x256 with the co-attention
 * mask).  Q/K/V are strided views into the fused projection output: row (b*T + t), columns
 * head*D .. head*D+D-1 from the given base pointer.  Tq, Tk <= 256; D in {64, 128}.
 * mask: bit-packed words [B][rows][ceil(Tk/32)] (unimm_mask_pack); mask_q_stride = 0 broadcasts
 * one row over all queries (key-padding mask).  lse (fp32 [B,H,Tq], log-sum-exp of the masked,
 * scaled scores) is what the backward kernels need; may be NULL for inference.
 * Variable-length ("unpadded") mode: when q_off/q_len (int32 [B], device) are given, sequence b owns
 * rows [q_off[b], q_off[b]+q_len[b]) of the packed q / out matrices (same for k_off/k_len and k, v);
 * Tq / Tk remain the PADDED lengths that index mask, lse and the dropout counters.  Padding rows
 * (fully masked queries that no valid row attends, models/vilbert_dialog.py:1418) are then never
 * computed at all.
 * Keys at positions >= k_len[b] (+ ks_len[b] when a shared segment is spliced in) do not exist, whatever their mask bits say,
 * and bits past Tk in a row's last word are ignored: only ceil(Tk/32) words of a mask row are read.
 * Alignment: q, k, v, out (and dq, dk, dv, dout of the backward) 16-byte aligned, every row stride a multiple of 8
 * elements: operand fragments are 16-byte loads and result rows leave as 16-byte stores; UNIMM_E_ALIGN otherwise.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  const void* q; const void* k; const void* v; /* bf16 */
  void* out;                                   /* bf16 [rows, ldo] */
  float* lse;
  const uint32_t* mask;
  const int32_t* q_off; const int32_t* q_len; const int32_t* k_off; const int32_t* k_len; /* or all NULL */
  int32_t B, H, Tq, Tk, D;
  int32_t ldq, ldk, ldv, ldo;
  int32_t mask_q_stride, mask_b_stride; /* in 32-bit words */
  float scale;
  uint32_t drop_key, drop_thr; float drop_scale;
  const uint32_t* drop_salt; /* or NULL (see unimm_gemm_nt_args.drop_salt) */ /* element index = ((b*H+h)*Tq+q)*Tk+k */
  /* unimm_attn_fwd and unimm_x3_attn_fwd only (NULL elsewhere), with k_off / k_len given and dropout off: a SHARED key/value segment -- rows
   * [ks_off[b], ks_off[b] + ks_len[b]) of the same k / v matrices -- spliced into sequence b's keys after its first ks_ins
   * private rows.  Key position j of sequence b is private row j (j < ks_ins), shared row j - ks_ins (j < ks_ins + ks_len[b]),
   * else private row j - ks_len[b]; the sequence has k_len[b] + ks_len[b] <= 256 keys and the mask words index key positions.
   * The position count is clamped to Tk, ks_len[b] < 0 is taken as 0, and nothing outside the two row ranges is read.
   * ks_off and ks_len come together or not at all; a segment without k_off / k_len, with ks_ins < 0 or with drop_thr != 0 is
   * UNIMM_E_ARG before any launch.  unimm_attn_bwd and unimm_x3_attn_bwd have no such fields and never take a segment: the training
   * pair of the spliced launch is unimm_attn_spliced_fwd / unimm_attn_spliced_bwd below.
   * Generative scoring (val_lm.py:52-121): the 100 candidate answers of a dialog round attend the round's context rows,
   * which are computed once (utils/data_utils.py:199-210: context rows never see the answer).  ABI 16. */
  const int32_t* ks_off; const int32_t* ks_len;
  int32_t ks_ins;
  /* or NULL: int32 [B], a permutation of 0..B-1 -- the order in which the launch's workgroups take the sequences (every head of
   * order[0] first).  Results do not depend on it; with variable lengths, longest first (unimm_plan_build writes that) keeps the
   * launch's tail short: +1 % on the 240-sequence step.  ABI 17.  (The fp32-class entry points honour it in their matrix-instruction kernels.) */
  const int32_t* order;
} unimm_attn_args;

int unimm_attn_fwd(const unimm_attn_args* args, void* stream);

/* The attention probabilities themselves, fp32 [B, H, Tq, Tk] (after dropout, as models/vilbert_dialog.py:401-405 /
 * :690-717 return them and BertEncoder collects them under output_all_attention_masks, :855-929).  Fixed layout only
 * (q_off .. k_len NULL); v / out / lse of the argument struct are ignored.  A diagnostic output, not part of the hot path:
 * unimm_attn_fwd never materialises them. */
int unimm_attn_probs(const unimm_attn_args* args, float* probs, void* stream);

/* Backward of unimm_attn_fwd (autograd of models/vilbert_dialog.py:390-410 / 519-539 / 681-721):
 * ONE launch for the text self-attention shape (D = 64, Tq and Tk above 64: dQ comes out of the dK / dV walk, `delta` is
 * then formed inside the kernel and the argument is left untouched); two launches on `stream` for the other shapes --
 * dQ (+ delta = rowsum(dO o O), fp32 [B,H,Tq] scratch) then dK/dV.
 * P is recomputed from Q, K and lse; the dropout mask is re-generated from (key, thr).
 * dq/dk/dv are bf16 strided views like q/k/v (typically into one [rows, 3*H*D] buffer). */
typedef struct {
  const void* q; const void* k; const void* v; const void* out; const void* dout; /* bf16 */
  const float* lse; float* delta;
  void* dq; void* dk; void* dv; /* bf16 */
  const uint32_t* mask;
  const int32_t* q_off; const int32_t* q_len; const int32_t* k_off; const int32_t* k_len; /* or all NULL */
  int32_t B, H, Tq, Tk, D;
  int32_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
  int32_t mask_q_stride, mask_b_stride;
  float scale;
  uint32_t drop_key, drop_thr; float drop_scale;
  const uint32_t* drop_salt;
  const int32_t* order;      /* as unimm_attn_args.order (ABI 17) */
} unimm_attn_bwd_args;

int unimm_attn_bwd(const unimm_attn_bwd_args* args, void* stream);

/* Training pair of the spliced launch (ABI 23): sequences whose private query rows attend their own rows and a SHARED key/value
 * segment (ks_off / ks_len / ks_ins above) -- N sampled answers of one dialog over the dialog's context rows, which are projected
 * once (unimm_amd/engine.py, the shared-context training step).
 * unimm_attn_spliced_fwd: unimm_attn_fwd's launch (same struct, same key-position rule, same kernels: with dropout off the two
 * are bit-identical) with lse required and attention dropout allowed; the dropout counter of (b, h, query q, key POSITION j) is
 * ((b*H+h)*Tq+q)*Tk+j as everywhere.
 * Limits of both: D = 64; Tq <= 32 (at most 32 private rows per sequence); Tk <= 256 and k_len[b] + ks_len[b] <= 256; q_off .. k_len,
 * ks_off and ks_len given; ks_ins >= 0.  Anything else: UNIMM_E_ARG (alignment: UNIMM_E_ALIGN, the rules above), before any launch.
 *
 * unimm_attn_spliced_bwd: the fields of unimm_attn_bwd_args, the segment, and the GROUPS of sequences that name the same segment:
 * g_seq (int32 [B], device) lists the launch's sequences group by group, g_first (int32 [G+1]) is where each group starts in it.
 * Members of a group need not be adjacent in the batch.  The group's segment is that of its first member with ks_len > 0; a member
 * with ks_len <= 0 attends its private rows only and adds nothing to the segment's rows.
 *   dq          rows of each sequence's private queries
 *   dk / dv     rows of each sequence's private keys, written once;
 *               rows of each group's segment: the sum over the group's sequences, accumulated in fp32 and rounded to bf16 ONCE.
 *               accumulate != 0: that one rounding is of (what the rows hold + the sum) -- the S x S self-attention backward
 *               (unimm_attn_bwd over the segments) writes its dk / dv into the same rows first.
 * P is recomputed from Q, K and lse, the dropout mask from the key, delta = rowsum(dO o out) of the GIVEN out inside the kernel:
 * `delta` and `order` are not read (a workgroup is one (group, head): list the largest groups first).  One workgroup walks its group's
 * sequences in list order and holds the segment's dK / dV in registers: no atomics, the same bits on every launch (4 of its 256 registers are spilled: 20 bytes of scratch per lane).
 * A segment no listed sequence names gets nothing written. */
int unimm_attn_spliced_fwd(const unimm_attn_args* args, void* stream);
typedef struct {
  const void* q; const void* k; const void* v; const void* out; const void* dout; /* bf16 */
  const float* lse; float* delta;
  void* dq; void* dk; void* dv; /* bf16 */
  const uint32_t* mask;
  const int32_t* q_off; const int32_t* q_len; const int32_t* k_off; const int32_t* k_len;
  int32_t B, H, Tq, Tk, D;
  int32_t ldq, ldk, ldv, ldo, lddo, lddq, lddk, lddv;
  int32_t mask_q_stride, mask_b_stride;
  float scale;
  uint32_t drop_key, drop_thr; float drop_scale;
  const uint32_t* drop_salt;
  const int32_t* order;
  const int32_t* ks_off; const int32_t* ks_len;
  int32_t ks_ins;
  const int32_t* g_first; const int32_t* g_seq;
  int32_t G;
  int32_t accumulate;
} unimm_attn_spliced_bwd_args;
int unimm_attn_spliced_bwd(const unimm_attn_spliced_bwd_args* args, void* stream);

/* The same pair for up to 64 private rows per sequence (added under ABI 24: two new entry points, no signature or struct changed, so
 * unimm_version() keeps its value): an answer of up to 30 tokens has 1 + 2 (30 + 1) = 63 private rows
 * (unimm_amd/scoring.py).  The argument structs, the key-position rule (ks_ins included), the group lists, `accumulate` and every
 * property of the results are those of the pair above; so is what is not read (`delta`, `order`).
 * Limits of both: D = 64; 1 <= Tq <= 64; Tk <= 256; k_len[b] <= 64 and k_len[b] + ks_len[b] <= 256; q_off .. k_len, ks_off and ks_len
 * (and g_first, g_seq, G >= 1 for the backward) given; ks_ins >= 0.  Anything else in the HOST arguments: UNIMM_E_ARG (alignment:
 * UNIMM_E_ALIGN) before any launch, nothing written.  The per-sequence lengths live in device memory and are clamped by the kernels
 * (q_len to min(Tq, 64), k_len to 64, the segment to 256 rows, group members to [0, B)): a bad length cannot make a launch touch rows
 * the arguments do not name.
 * lse is [B, H, Tq] and the dropout counters are those of the padded (B, H, Tq, Tk) box with the Tq PASSED: a launch with Tq = 64 does
 * not reproduce the dropout pattern of the Tq = 32 launch on the same sequences.
 * unimm_attn_spliced_wide_fwd: unimm_attn_fwd's launch once more (two query tiles per sequence; without dropout bit-identical to it).
 * unimm_attn_spliced_wide_bwd: a kernel of its own, one workgroup per (group, head).  Both query tiles of a sequence are staged at
 * once; a shared key tile's wave adds both into its fp32 dK / dV registers, held over the whole walk and rounded to bf16 once (with
 * `accumulate`, together with what the rows hold); each of the two private key tiles runs over both query tiles on one wave and is
 * rounded once per sequence.  No atomics, no workspace, the same bits on every launch.  159 KiB of LDS: one workgroup per CU, as for
 * the narrow kernel.  Measured once (profiles/README.md, r12a): 2.2x the narrow kernel's time at 20-token answers; not tuned. */
int unimm_attn_spliced_wide_fwd(const unimm_attn_args* args, void* stream);
int unimm_attn_spliced_wide_bwd(const unimm_attn_spliced_bwd_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Row kernels (HBM-bound).
 * ------------------------------------------------------------------------------------------- */
enum { UNIMM_DT_U8 = 0, UNIMM_DT_I32 = 1, UNIMM_DT_I64 = 2, UNIMM_DT_F32 = 3 };

/* Bit-pack a 0/1 mask [rows, t] (bool/uint8, int32, int64 or fp32; nonzero = attend) into
 * ceil(t/32) words per row.  Replaces the fp32 (1-m)*-10000 mask tensors of
 * models/vilbert_dialog.py:1415-1431 (the -10000 is applied inside the attention kernels). */
int unimm_mask_pack(const void* mask, int dtype, uint32_t* out, int64_t rows, int32_t t, void* stream);
/* The same words computed on the HOST (ABI 18; no device work, no stream): `mask` and `out` are host pointers.  The reference's
 * callers pass CPU tensors to forward() (train.py:113-129; utils/data_parallel.py:123-124 scatters them) -- int64 [B, 256, 256]
 * masks, 512 KiB per sequence; packed on the host side of the copy, 8 KiB per sequence cross PCIe.  threads: 0 = up to 16. */
int unimm_host_mask_pack(const void* mask, int dtype, uint32_t* out, int64_t rows, int32_t t, int32_t threads);
/* memcpy between two HOST buffers on `threads` threads (0 = up to 8): the caller's pageable tensors -> the pinned staging ring the
 * asynchronous host->device copies read (one thread moves the 130 MB of region features / targets of a 240-sequence batch in
 * ~25 ms: most of a step; torch's copy_ depends on the size of torch's intra-op pool).  ABI 18. */
int unimm_host_memcpy(void* dst, const void* src, int64_t bytes, int32_t threads);
/* The same words without the dense mask: the text mask [B, T, ceil(T/32)] and the
 * co-attention key mask [B, ceil(T/32)] (one row per sequence, mask_q_stride = 0) of B sequences from three
 * int32 device arrays: mode (0 = discriminative, utils/data_utils.py:391-396; 1 = generative, :199-210),
 * len = L (tokens up to and including the answer's [SEP]; L <= T) and nans = n (answer length + 1, the size
 * of the [MASK]-copy block; ignored when mode = 0).  Removes the 512 KiB per sequence of int64 mask the
 * reference ships to the device. */
int unimm_mask_synth(const int32_t* mode, const int32_t* len, const int32_t* nans, uint32_t* text_words, uint32_t* co_words,
                     int32_t B, int32_t T, void* stream);

/* Plan of the unpadded schedule, on the device (replaces ~25 eager kernels over the dense masks and two of the three
 * device->host round trips of a step).  unimm_plan_lengths: header[b] = valid prefix length of sequence b (>= 1; a token
 * is valid when it attends something, is attended by a token or a region, or carries a label / weight; a sequence with a
 * valid token whose own row of a dense text mask is empty gets its full length T, as that token attends all T keys), header[B+b] =
 * rows the MLM head decodes (weight != 0 when weights are given, else label != -1), header[2B..2B+1] = bit patterns of
 * the two NSP class weights when nsp_weight != NULL, header[2B+2+b] = regions of sequence b with image_label == 1
 * (int32 [B, R] or NULL: the divisor of the masked-region loss); header has 3B+2 entries.  Masks are the packed words of
 * unimm_mask_pack / unimm_mask_synth with their (query, batch) word strides (query stride 0 = one key-padding row per
 * sequence); text_words or co_words may be NULL, labels / weights int32 [B, T] or NULL.
 * unimm_plan_build (after the host has read the header and allocated): off[B] / lens[B], rows[sum len] = padded row of
 * every packed row, inv[B*T] = packed row or -1, and for the decoded rows, in row order, lm_pos (padded row), lm_idx
 * (packed row), lm_label, lm_weight (1 when weights == NULL); rows / inv / the lm_* group may be NULL. */
int unimm_plan_lengths(const uint32_t* text_words, int32_t t_q_stride, int32_t t_b_stride, const uint32_t* co_words,
                       int32_t c_q_stride, int32_t c_b_stride, int32_t R, const int32_t* labels, const int32_t* weights,
                       const float* nsp_weight, const int32_t* image_label, int32_t B, int32_t T, int32_t* header,
                       void* stream);
/* Replayed launch sequences (unimm_amd/graphs.py: the step as two hipGraphs): kernel ARGUMENTS are frozen at capture, so a
 * launch is sized for a CAPACITY (the step's row counts rounded up to a bucket) and every kernel whose result would change
 * with the surplus rows reads the REAL count from device memory (the `*_dev` arguments below and in the structs above;
 * NULL = the argument is exact).  unimm_plan_build writes those words: dims_i = {valid text rows, decoded rows, regions in
 * the masked-region loss}, dims_f = {1 / decoded rows, 1 / regions (inf when none, as the reference's division)}; it also
 * fills rows[real .. rows_cap) and the lm_* lists [real .. lm_cap) with safe values (index 0, label -1, weight 0) so that
 * row-independent kernels (GEMM, LayerNorm forward, gathers) may run over the whole capacity.  dims_i (>= 4 words) / dims_f
 * (>= 2) both or neither.  Capacities are REQUIRED: rows_cap is the length of rows whenever rows is given, lm_cap that of the lm_*
 * lists whenever they are given, and a list with a capacity <= 0 is refused (UNIMM_E_ARG, nothing is launched); for an exact
 * plan pass the header's own totals (capacities >= the counts; a capacity is ignored when its list is NULL).  With no decoded
 * row dims_f[0] = 1.  A batch whose real counts EXCEED a capacity (a replayed step sized
 * from a stale header) never writes past the lists: indices and the counts in dims_i are clamped to the capacities,
 * dims_i[3] = 1 and both dims_f words are NaN (the step's losses come out NaN instead of memory being corrupted). */
int unimm_plan_build(const int32_t* header, const int32_t* labels, const int32_t* weights, int32_t B, int32_t T,
                     int32_t* off, int32_t* lens, int64_t* rows, int64_t* inv, int32_t* lm_pos, int32_t* lm_idx,
                     int32_t* lm_label, int32_t* lm_weight, int32_t rows_cap, int32_t lm_cap, int32_t* dims_i, float* dims_f,
                     int32_t* order, void* stream);
/* order (ABI 17; or NULL): int32 [B] = the sequences by valid length, longest first (ties in batch order): what
 * unimm_attn_args.order takes. */

/* y = LayerNorm(x) (eps inside sqrt, torch.nn.LayerNorm; models/vilbert_dialog.py:279) with optional
 * dropout on y.  The residual stream is fp32 (as under the reference's autocast, where layer_norm and
 * the residual add run in fp32): x fp32 [M, H]; y32 (fp32, next residual) and / or y16 (bf16, next GEMM
 * operand) are written; mean/rstd fp32 [M] saved for backward (may be NULL). */
int unimm_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y32, void* y16, float* mean,
                        float* rstd, int32_t M, int32_t H, float eps, uint32_t drop_key, uint32_t drop_thr,
                        float drop_scale, const uint32_t* drop_salt, void* stream);

/* bytes of the `partials` scratch the two backward row kernels need for hidden size H */
int64_t unimm_colpartials_bytes(int32_t H);

/* LayerNorm backward (dy bf16, x = the fp32 pre-LayerNorm sum).  dx (bf16) is the gradient w.r.t. the pre-LayerNorm sum (= the residual
 * branch gradient); dx_drop (optional) = dropout-masked dx for the dense branch (drop_*: the mask the
 * forward GEMM epilogue applied); odrop_*: dropout applied to y in the forward (embeddings), 0 = none.
 * dgamma/dbeta/dbias (fp32 [H], any may be NULL) are ACCUMULATED (+=); dbias = colsum(dx_drop). */
int unimm_layernorm_bwd(const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                        void* dx, void* dx_drop, float* dgamma, float* dbeta, float* dbias, float* partials,
                        int32_t M, int32_t H, uint32_t drop_key, uint32_t drop_thr, float drop_scale,
                        uint32_t odrop_key, uint32_t odrop_thr, float odrop_scale, const uint32_t* drop_salt,
                        const int32_t* drop_rows, void* stream);
/* The same row kernel without the reduction of its column partials: `partials` (unimm_colpartials_bytes(H), private to
 * this call until it is reduced) holds [blocks][3][H] = per-block sums for dgamma, dbeta, dbias; *blocks_out (host)
 * receives the block count.  unimm_colpartials_finish_grouped then adds the column sums of up to many pending calls
 * into their destinations in one launch (dst[q] == NULL skips quantity q): the engine reduces a block's LayerNorm
 * partials once at the end of the block instead of between two dependent kernels each time.  m_dev (or NULL): device word with
 * the rows actually present (M = capacity); rows at or past it are neither read nor written and add nothing to the partials.
 * drop_rows (both entry points; int32 [M] or NULL = the identity): row m draws both dropout masks (drop_*, odrop_*) as row
 * drop_rows[m] -- the rows of a gathered block keep the masks of the rows they came from (unimm_gemm_nt_args.drop_rows). */
int unimm_layernorm_bwd_partials(const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                 void* dx, void* dx_drop, float* partials, int32_t M, int32_t H, uint32_t drop_key,
                                 uint32_t drop_thr, float drop_scale, uint32_t odrop_key, uint32_t odrop_thr,
                                 float odrop_scale, int32_t* blocks_out, const int32_t* m_dev, const uint32_t* drop_salt,
                                 const int32_t* drop_rows, void* stream);
#define UNIMM_FINISH_MAX 8
typedef struct {
  const float* partials;
  float* dst[4];
  int32_t blocks, nq, H, pad_;
} unimm_finish_desc;
int unimm_colpartials_finish_grouped(const unimm_finish_desc* descs, int32_t count, void* stream);

/* Text embeddings: y = dropout(LN(word[ids] + pos[position] + type)) with token-type ids >= type_vocab
 * routed to the 10-row extension table (BertEmbeddingsDialog.forward, models/vilbert_dialog.py:326-356).
 * Tables are the fp32 master weights; ids int32 [M]; y32 / y16 as for unimm_layernorm_fwd. */
typedef struct {
  const int32_t* ids; const int32_t* pos; const int32_t* typ;
  const float* word; const float* post; const float* type; const float* ext; /* fp32 tables, row length H */
  const float* gamma; const float* beta;
  int32_t M, H, type_vocab;
  float eps;
  uint32_t drop_key, drop_thr; float drop_scale;
  const int32_t* m_dev; /* or NULL: device word with the rows actually present (M = capacity); later rows are not read or written */
  const int64_t* rows;  /* or NULL: row r takes ids / pos / typ at index rows[r] (the unpadded schedule's row map) */
  const uint32_t* drop_salt; /* or NULL (see unimm_gemm_nt_args.drop_salt) */
} unimm_embed_args;

int unimm_embed_fwd(const unimm_embed_args* args, float* y32, void* y16, void* stream);
/* backward: re-gathers the rows, LayerNorm backward, scatter-add (fp32 atomics) into the word /
 * position / extension-type gradient tables; dtype [2, H], dgamma, dbeta accumulated via partials. */
int unimm_embed_bwd(const unimm_embed_args* args, const void* dy, float* dword, float* dpos, float* dtype,
                    float* dext, float* dgamma, float* dbeta, float* partials, void* stream);
/* The same without the atomics (ABI 23): the gradient of every embedded row is STORED in drow (fp32 [M, H]) and no table is
 * touched; dtype, dgamma, dbeta as above.  unimm_rows_scatter_sum_f32 then adds the rows into a table in a fixed order:
 * dst[keys[j]] += src[order[j]] over the list positions j of one key, one writer per destination row, the addends in a fixed order
 * (eight interleaved partial sums in list order, then added in order) -- keys int32 [M] ascending (negative or >= n_dst: skipped)
 * and order int32 [M] as a stable sort of the rows' table indices gives them; H <= 1024 (UNIMM_E_SHAPE).  The
 * embedding gradient of the shared-context training step: a step repeats bit for bit. */
int unimm_embed_bwd_rows(const unimm_embed_args* args, const void* dy, float* drow, float* dtype, float* dgamma, float* dbeta,
                         float* partials, void* stream);
int unimm_rows_scatter_sum_f32(const float* src, const int32_t* keys, const int32_t* order, int32_t M, int32_t H, float* dst,
                               int32_t n_dst, void* stream);

/* db[N] += column sums of dy (bf16 [M, N], row stride ld): bias gradients. */
int unimm_colsum(const void* dy, float* db, int32_t M, int32_t N, int32_t ld, void* stream);

/* fp32 -> bf16 weight copies: flat cast, and dst[c][r] = src[r][c] (dst row stride ldd >= R, columns
 * R..ldd-1 zero-filled) for the transposed copies the input-gradient GEMMs read. */
int unimm_cast_f32_bf16(const float* src, void* dst, int64_t n, void* stream);
int unimm_transpose_cast(const float* src, void* dst, int32_t R, int32_t C, int32_t ldd, void* stream);
/* bf16 -> bf16 transpose: dst[c][r] = src[r][c]; src [R, C] row stride lds, dst [C, ldd] with columns R..ldd-1
 * zero-filled; lds, ldd multiples of 8, both pointers 16-byte aligned.  Puts the decoder-logit gradient of
 * models/vilbert_dialog.py:1023-1026 reduction-major so that its input gradient (a few hundred rows x 768 over the
 * 30,522-long vocabulary axis) can run as a split reduction on unimm_gemm_tn_grouped. */
int unimm_transpose_bf16(const void* src, void* dst, int32_t R, int32_t C, int32_t lds, int32_t ldd, void* stream);
/* out[i] (bf16) = slabs[0][i] + slabs[1][i] + ... + slabs[count-1][i] (fp32, in that order), i < n; slab s starts at
 * slabs + s * stride.  n a multiple of 8, stride of 4, 16-byte aligned pointers.  The fixed-order reduction of the
 * per-chunk partial sums of the split decoder input gradient (see unimm_transpose_bf16). */
int unimm_sum_slabs_bf16(const float* slabs, int32_t count, int64_t stride, void* out, int64_t n, void* stream);
/* Segmented sum of row BLOCKS (ABI 23): src holds n_items blocks of R rows x W bf16 (row stride lds), block g of dst (R rows, row
 * stride ldd) = the sum of the blocks items[first[g]] .. items[first[g + 1] - 1], added in fp32 in list order, rounded once; first
 * int32 [G + 1], items int32 (device).  W, lds, ldd multiples of 8, 16-byte aligned pointers.  The region gradients of the
 * shared-context training step: every text block of a group attends the group's regions, the text-attends-regions backward
 * writes one copy of dK / dV per block and this adds a group's copies up -- the same bits on every run. */
int unimm_segment_rows_sum_bf16(const void* src, int32_t lds, const int32_t* first, const int32_t* items, int32_t n_items,
                                int32_t G, void* dst, int32_t ldd, int32_t R, int32_t W, void* stream);
/* The same for `count` matrices in one launch.  `table` is a DEVICE array; entry i owns blocks
 * [tile0_i, tile0_{i+1}) with ceil(C/32) * ceil(ldd/32) blocks each (tile0 ascending, tile0_0 = 0);
 * total_tiles = their sum.  Used after the optimizer step to rebuild every transposed weight copy. */
typedef struct {
  const float* src;  /* fp32 [R, C] */
  void* dst;         /* bf16 [C, ldd] */
  int32_t R, C, ldd, tile0;
} unimm_transpose_desc;
int unimm_transpose_cast_grouped(const unimm_transpose_desc* table, int32_t count, int32_t total_tiles, void* stream);

/* Region features fp32 [rows, F] + box geometry fp32 [rows, 5] -> bf16 [rows, ld] = [feat | loc | 0]:
 * the operand of the single image-embedding GEMM (models/vilbert_dialog.py:1488-1489). */
int unimm_pack_image(const float* feat, const float* loc, void* out, int32_t rows, int32_t F, int32_t ld, void* stream);

/* out = dropout(a * b) (pooled_t * pooled_v, models/vilbert_dialog.py:1065), fp32 flat [n], and its backward, which
 * also folds in the pooler ReLU gradient (:951, :966): da = [a>0] drop(dout) b, db = [b>0] drop(dout) a. */
int unimm_mul_dropout(const float* a, const float* b, float* out, int64_t n, uint32_t drop_key, uint32_t drop_thr,
                      float drop_scale, const uint32_t* drop_salt, void* stream);
int unimm_mul_dropout_bwd(const float* a, const float* b, const float* dout, float* da, float* db, int64_t n,
                          uint32_t drop_key, uint32_t drop_thr, float drop_scale, const uint32_t* drop_salt, void* stream);

/* The same for fusion_method = 'sum' (models/vilbert_dialog.py:1062-1063): out = dropout(a + b); da = [a>0] drop(dout),
 * db = [b>0] drop(dout). */
int unimm_sum_dropout(const float* a, const float* b, float* out, int64_t n, uint32_t drop_key, uint32_t drop_thr,
                      float drop_scale, const uint32_t* drop_salt, void* stream);
int unimm_sum_dropout_bwd(const float* a, const float* b, const float* dout, float* da, float* db, int64_t n,
                          uint32_t drop_key, uint32_t drop_thr, float drop_scale, const uint32_t* drop_salt, void* stream);

/* fp32 linear algebra of the heads on top of the network (the two poolers :946-967, the NSP head :1070) and their
 * backward, on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32, straight from the fp32 master weights:
 *   OUT[m, n] (+)= act( sum_k A(m, k) * B(k, n) + bias[n] ),  A(m, k) = a[m * sa_m + k * sa_k],  B(k, n) = b[k * sb_k + n * sb_n]
 * (strides in elements), act = ReLU when relu != 0; accumulate != 0 adds into OUT with fp32 atomics (gradients
 * accumulate); rowsum (or NULL): rowsum[m] += sum_k A(m, k), the bias gradient when A = dY^T.  One kernel gives
 *   y = x W^T + b   (a = x: sa_m = ldx, sa_k = 1;  b = W [N, K]: sb_k = 1, sb_n = ldw),
 *   dx = dy W        (a = dy: sa_m = lddy, sa_k = 1;  b = W: sb_k = ldw, sb_n = 1),
 *   dW += dy^T x     (a = dy: sa_m = 1, sa_k = lddy;  b = x: sb_k = ldx, sb_n = 1;  M = out features, K = batch rows). */
typedef struct {
  const float* a; const float* b; const float* bias; float* out; float* rowsum;
  int32_t M, N, K;
  int64_t sa_m, sa_k, sb_k, sb_n, ldo;
  int32_t relu, accumulate;
} unimm_linear_f32_args;
int unimm_linear_f32(const unimm_linear_f32_args* args, void* stream);
/* dst[idx[r], :] += src[r, :]: bf16 rows of H elements, fp32 addend, idx unique (the pooler input gradient joins the
 * gradient of the first-token rows, models/vilbert_dialog.py:949, :964). */
int unimm_rows_add_f32(void* dst, const int32_t* idx, const float* src, int32_t n, int32_t H, void* stream);

/* du = dt * GELU'(u), bf16 flat [n], n % 8 == 0 (prediction-head transforms, :983-985, :1002-1004) */
int unimm_gelu_bwd(const void* dt, const void* u, void* du, int64_t n, void* stream);
/* scatter == 0: dst[i,:] = src[idx[i],:]; scatter != 0: dst[idx[i],:] = src[i,:]  (bf16 rows of H, idx unique).
 * Selects the labelled token rows the decoder runs on (the reference decodes all 256 rows and then
 * boolean-gathers, models/vilbert_dialog.py:1583-1584).  n_dev (or NULL): device word with the rows actually present (n = capacity);
 * rows i at or past it are not read, and the rows they would write are left untouched. */
int unimm_gather_rows(const void* src, const int32_t* idx, void* dst, int32_t n, int32_t H, int32_t scatter,
                      const int32_t* n_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Losses.  Row kernels (one workgroup per row) keep logits, log-sum-exp and 1-p in fp32.
 * `g` is a DEVICE pointer to the upstream gradient of the (shape-[1]) loss; inv_denom a host float.
 * ------------------------------------------------------------------------------------------- */
/* Token-level likelihood / unlikelihood (models/vilbert_dialog.py:1577-1595): per decoded row with
 * label y (-1 = ignore) and integer weight w: w>0 -> -w*log p_y; w==-1 -> -log(clamp(1-p_y, 1e-6)).
 * rowloss is the un-normalised contribution, rownll = -log p_y (generative scoring, val_lm.py:131-136),
 * lse the row's log-sum-exp.  The :1600-1604 CrossEntropy fallback is this with w = [y != -1].  n_dev (or NULL): device word with
 * the rows actually present (n = capacity); rows at or past it are neither read nor written. */
int unimm_lm_loss_fwd(const float* logits, const int32_t* labels, const int32_t* weights, float* rowloss,
                      float* rownll, float* lse, int32_t n, int32_t V, int32_t ld, const int32_t* n_dev, void* stream);
/* dlogits (bf16 [n, ldd], columns >= V zero-filled) = g * inv_denom * d(rowloss)/d(logits); inv_dev (or NULL): the
 * denominator's reciprocal as a device word instead of the host float; n_dev as for the forward (rows past it: dlogits untouched) */
int unimm_lm_loss_bwd(const float* logits, const int32_t* labels, const int32_t* weights, const float* lse,
                      const float* g, float inv_denom, void* dlogits, int32_t n, int32_t V, int32_t ld,
                      int32_t ldd, const int32_t* n_dev, const float* inv_dev, void* stream);
/* Policy-gradient objective on decoded rows of SAMPLED answers (csrc/policy.hip, ABI 22; an extension: self-critical /
 * importance-weighted fine-tuning on a sequence-level reward).  logits, labels, lse, rownll, n / n_dev / inv_dev, ld / ldd and
 * the zero-filled columns >= V are those of unimm_lm_loss_*; V <= 65536.  The row's advantage A and behaviour log-probability
 * b are read by the kernel: A = adv[pos[row]], b = blogp[pos[row]] (pos = the row's flat position b * T + t; pos == NULL:
 * adv[row], blogp[row]); adv / blogp hold n_adv floats and a position outside [0, n_adv) makes the row an ignored one.
 * With logp = z_y - lse and H = -sum_i p_i log p_i:
 *   mode 0 (LOGP):   surr = A logp                                         (blogp is not read and may be NULL)
 *   mode 1 (RATIO):  r = exp(logp - b), surr = min(r A, clamp(r, 1 - clip_eps, 1 + clip_eps) A)   (clip_eps = +inf: unclipped)
 *   rowloss = -surr - beta H;  A == 0 gives surr = 0 whatever logp is;  ent = H is written for every row
 *   label < 0:  rowloss = rownll = 0 and an all-zero gradient row (also with beta != 0)
 * H comes out of the log-sum-exp pass (H = lse - sum_i e^(z_i - m) z_i / sum_i e^(z_i - m)): each logit is read once per
 * direction; a -inf logit has p = 0 and contributes 0 to H and to its gradient.
 *   dlogits[row, i] = g inv ( c (p_i - [i == y]) + beta p_i (log p_i + H) ),  c = A (LOGP);  c = A r (RATIO), or 0 where the
 *   clipped branch is the strict minimum (A > 0 and r > 1 + clip_eps, or A < 0 and r < 1 - clip_eps).
 * With beta = 0 and mode 0 both directions equal unimm_lm_loss_* with weight w = A bit for bit (A a positive integer). */
int unimm_pg_loss_fwd(const float* logits, const int32_t* labels, const int32_t* pos, const float* adv, const float* blogp,
                      int32_t n_adv, int32_t mode, float clip_eps, float beta, float* rowloss, float* rownll, float* lse,
                      float* ent, int32_t n, int32_t V, int32_t ld, const int32_t* n_dev, void* stream);
int unimm_pg_loss_bwd(const float* logits, const int32_t* labels, const int32_t* pos, const float* adv, const float* blogp,
                      int32_t n_adv, int32_t mode, float clip_eps, float beta, const float* lse, const float* ent,
                      const float* g, float inv_denom, void* dlogits, int32_t n, int32_t V, int32_t ld, int32_t ldd,
                      const int32_t* n_dev, const float* inv_dev, void* stream);
/* The same objective with a per-row penalty kl_coef KL(p || pr) against a FROZEN reference (two entry points added beside the
 * pair above, whose signatures and results are unchanged: the ABI number stays).  ref_logits: the reference's fp32 rows for
 * the same n decoded rows, V valid columns, row stride ld_ref >= V, independent of ld.  With p = softmax(z), pr = softmax(zr):
 *   KL      = sum_i p_i (log p_i - log pr_i)
 *   rowloss = (unimm_pg_loss_fwd's) + kl_coef KL
 *   dlogits[row, i] = g inv ( (unimm_pg_loss_bwd's three terms) + kl_coef p_i (log p_i - log pr_i - KL) );  nothing flows into
 *   the reference.
 * kl and ref_lse (the reference row's log-sum-exp) are written by the forward and read by the backward; ref_lse is written for
 * every row, kl is 0 on an ignored row (label < 0 or a position outside [0, n_adv)), whose rowloss, rownll and gradient row are
 * exactly zero whatever kl_coef is.  A == 0 switches neither the entropy term nor the KL term off.  n_dev, inv_dev, pos, V <=
 * 65536 and the zero-filled columns V .. ldd: as above; rows past n_dev[0] are neither read nor written (kl, ref_lse included).
 * One pass per direction: the forward keeps u = sum_i e^(z_i - m)(z_i - zr_i) and the reference row's own (mr, sr) beside the
 * policy row's (m, s, t), and KL = u / s - lse + ref_lse; the backward uses log p_i - log pr_i = (z_i - lse) - (zr_i - ref_lse).
 * Each row is read once per direction.  The backward reads each row with 16-byte loads when that row's own stride is a
 * multiple of 4 floats; the forward walks both rows in the policy row's column order, so there the reference row's 16-byte
 * loads also need ld % 4 == 0 (a policy row on the scalar path reads both rows one column at a time).
 * -inf: a policy logit of -inf has p_i = 0 and contributes exactly 0 to KL and to its gradient element, whatever zr_i holds
 * (finite or -inf).  zr_i = -inf where z_i is finite is OUTSIDE the contract (the engine's decoder never produces it): that
 * row's kl, rowloss and gradient are then unspecified (inf / NaN); every other row is unaffected.
 * Bit-exact: (1) lse, ent and rownll, and with kl_coef = 0 also rowloss and dlogits, equal unimm_pg_loss_fwd / _bwd on the same
 * arguments bit for bit (one template; the KL term is an addend of its own).  (2) With ref_logits == logits and ld_ref == ld,
 * KL is exactly +0, ref_lse == lse bitwise (the reference row's log-sum-exp takes the policy row's operation sequence) and
 * dlogits equals unimm_pg_loss_bwd's bit for bit for any kl_coef (a zero KL term is not added).
 * UNIMM_E_ARG before any launch: ref_logits, kl or ref_lse NULL, ld_ref < V, kl_coef negative or not finite; the refusals of
 * the pair above apply as well. */
int unimm_pg_kl_loss_fwd(const float* logits, const int32_t* labels, const int32_t* pos, const float* adv, const float* blogp,
                         int32_t n_adv, int32_t mode, float clip_eps, float beta, float* rowloss, float* rownll, float* lse,
                         float* ent, int32_t n, int32_t V, int32_t ld, const int32_t* n_dev, const float* ref_logits,
                         int32_t ld_ref, float kl_coef, float* kl, float* ref_lse, void* stream);
int unimm_pg_kl_loss_bwd(const float* logits, const int32_t* labels, const int32_t* pos, const float* adv, const float* blogp,
                         int32_t n_adv, int32_t mode, float clip_eps, float beta, const float* lse, const float* ent,
                         const float* g, float inv_denom, void* dlogits, int32_t n, int32_t V, int32_t ld, int32_t ldd,
                         const int32_t* n_dev, const float* inv_dev, const float* ref_logits, int32_t ld_ref, float kl_coef,
                         const float* kl, const float* ref_lse, void* stream);
/* Token-level knowledge distillation against a FROZEN teacher (csrc/distill.hip; two entry points added beside the ones above,
 * whose signatures and results are unchanged: the ABI number stays).  logits, labels, weights, lse, rownll, n / n_dev / inv_dev,
 * ld / ldd and the zero-filled columns V .. ldd are those of unimm_lm_loss_*; V <= 65536.  ref_logits: the teacher's fp32 rows
 * for the same n decoded rows, V valid columns, row stride ld_ref >= V, independent of ld.  With temperature tau > 0, hard-label
 * share alpha in [0, 1], p = softmax(z / tau), q = softmax(zr / tau):
 *   hard    = unimm_lm_loss_fwd's rowloss for (y, w)
 *   KD      = KL(q || p) = sum_i q_i (log q_i - log p_i)
 *   rowloss = alpha hard + (1 - alpha) tau^2 KD
 *   dlogits[row, i] = g inv ( alpha (unimm_lm_loss_bwd's element) + (1 - alpha) tau (p_i - q_i) );  nothing flows into the teacher.
 * A row takes part when y >= 0 and w > 0 or w == -1 (the weights unimm_lm_loss_fwd gives a loss for).  A row that takes no
 * part has rowloss = kd = 0 and a gradient row of +0 (rownll is still -log p_y where y >= 0, as unimm_lm_loss_fwd writes it).
 * Forward, one pass over both rows: beside the student row's running maximum m and s = sum e^(z_i - m) a lane keeps
 * st = sum e^((z_i - m) / tau), and for the teacher row its own mr, sr = sum e^((zr_i - mr) / tau) and
 * ur = sum e^((zr_i - mr) / tau) (zr_i - z_i); then lse = m + log s, lse_t = m / tau + log st, ref_lse_t = mr / tau + log sr and
 * KD = ur / (sr tau) - ref_lse_t + lse_t.  It writes rowloss, rownll, lse, lse_t, ref_lse_t and kd (kd: 0 on a row that takes no
 * part; the log-sum-exps: every row below the count).  Backward: p_i - q_i = e^(z_i / tau - lse_t) - e^(zr_i / tau - ref_lse_t); a
 * row whose two coefficients are both zero (no part; alpha == 1 with a clamped unlikelihood; g == 0) is filled with +0 without a
 * logit being read.  Each row is read once per direction.  The backward reads each row with 16-byte loads when that row's own
 * stride is a multiple of 4 floats; the forward walks both rows in the student row's column order, so there the teacher row's
 * 16-byte loads also need ld % 4 == 0 (a student row on the scalar path reads both rows one column at a time).
 * -inf: a teacher logit of -inf has q_i = 0 and contributes exactly 0 to KD and to the gradient element, whatever z_i holds
 * (finite or -inf); a student logit of -inf has p_i = 0 (on the label the hard term is +inf, and so is rowloss unless alpha == 0:
 * a share of exactly 0 or 1 adds nothing of the other term, never 0 * inf).  z_i = -inf where zr_i is finite is OUTSIDE the contract (the engine's
 * decoder never produces it): that row's KD is +inf and its rowloss and gradient are unspecified (inf / NaN); every other row is
 * unaffected.
 * Bit-exact: (1) rownll and lse equal unimm_lm_loss_fwd's on the same arguments bit for bit ((m, s) take its operation
 * sequence) on every row it defines: a row that holds -inf logits can come out of unimm_lm_loss_fwd as NaN (e^(-inf - -inf)),
 * here it is finite and equals unimm_pg_loss_fwd's.  (2) With alpha == 1 the soft term is not added and the teacher row is not
 * read (ref_logits may be NULL; ref_lse_t and kd are written as 0): rowloss and dlogits equal unimm_lm_loss_fwd / _bwd bit for bit
 * for every weight, -1 included, except that a row whose coefficient is zero is +0 throughout where unimm_lm_loss_bwd leaves -0
 * on its label.  (3) With ref_logits == logits and ld_ref == ld, kd is exactly +0 and ref_lse_t == lse_t bitwise for any tau (the
 * teacher row's log-sum-exp takes the student row's operation sequence), and the soft term's gradient elements are exactly
 * zero.  (4) With tau == 1, lse_t == lse bitwise.
 * UNIMM_E_ARG before any launch: a NULL pointer (ref_logits only when alpha != 1; n_dev and inv_dev may be NULL), ld_ref < V
 * with a teacher given, tau not finite or <= 0, alpha outside [0, 1] or NaN; UNIMM_E_SHAPE as for unimm_lm_loss_*, and V > 65536. */
int unimm_distill_loss_fwd(const float* logits, const int32_t* labels, const int32_t* weights, const float* ref_logits,
                           int32_t ld_ref, float tau, float alpha, float* rowloss, float* rownll, float* lse, float* lse_t,
                           float* ref_lse_t, float* kd, int32_t n, int32_t V, int32_t ld, const int32_t* n_dev, void* stream);
int unimm_distill_loss_bwd(const float* logits, const int32_t* labels, const int32_t* weights, const float* ref_logits,
                           int32_t ld_ref, float tau, float alpha, const float* lse, const float* lse_t, const float* ref_lse_t,
                           const float* g, float inv_denom, void* dlogits, int32_t n, int32_t V, int32_t ld, int32_t ldd,
                           const int32_t* n_dev, const float* inv_dev, void* stream);
/* Listwise preference objective on the likelihoods of whole candidate answers (csrc/policy.hip; an entry point added beside the
 * ones above, whose signatures and results are unchanged: the ABI number stays).  It sits between unimm_lm_loss_fwd, which leaves
 * rownll = -log p_y per decoded row, and unimm_pg_loss_bwd in LOGP mode, which turns a per-row coefficient A into the gradient of
 * -A log p_y: per-row log-probabilities become per-sequence scores, the sequences of a group (a dialog) are compared with each
 * other and with a frozen reference, and every row gets its sequence's coefficient.
 * Row r < min(n, *n_dev) belongs to sequence row_seq[r]; sequence j to group seq_group[j] with target weight seq_weight[j] >= 0.
 * M_g = the sequences of group g that have at least one row.  For j in M_g, in fp64:
 *   S_j = -sum_r rownll[r],  R_j = -sum_r ref_rownll[r] (0 without a reference),  L_j = number of rows of j
 *   D_j = (S_j - R_j) / L_j^lam (lam = 1 if length_normalize else 0),  z_j = beta D_j
 *   logP_j = z_j - logsumexp_{k in M_g} z_k,  P_j = exp(logP_j),  W_g = sum_{j in M_g} w_j
 *   group_loss[g] = -sum_{j in M_g} w_j logP_j,  c_j = beta (w_j - W_g P_j) / L_j^lam = -d group_loss[g] / d S_j
 * A group is ALIVE when W_g > 0; the caller's loss is sum(group_loss) * alive_inv[0].  Two candidates with w = (1, 0) give
 * -log sigmoid(z_w - z_l) (DPO); softmax(relevance) as w gives the ListNet top-1 form.
 * Outputs (fp32, each rounded from fp64 once): adv[r] = c_j on every row of j (0 on the rows of a group that is not alive),
 * seq_score[j] = D_j (NaN for a sequence without rows), seq_prob[j] = P_j (0 for a sequence without rows or outside every
 * group), group_loss[g] (0 for a group that is not alive), alive_inv[0] = 1 / #alive (NaN when none): alive_inv can serve as
 * the inv_dev / scale_dev word of unimm_pg_loss_bwd and unimm_reduce_sum.
 * Order: a sequence's rows are added in ascending row index, a group's members are taken in ascending sequence index, every
 * sum is a serial chain of fp64 additions in that order.  No float atomics, no arrival counters: the same inputs give the same
 * bits.  row_seq need not be sorted or contiguous.  Three launches: per sequence (one wave each), per group (one workgroup
 * each, the members' z, w and L in LDS), per row.
 * Values the host cannot see never lead out of a buffer: a row_seq outside [0, B) makes the row an ignored one (adv = 0); a
 * seq_group outside [0, groups) takes the sequence out of every group (its seq_score is still written, seq_prob = 0, adv = 0);
 * a group with more than UNIMM_PREF_MAX_MEMBERS members, or with a member whose weight is negative or not finite, is not alive
 * and has group_loss = NaN, its members seq_prob = NaN and adv = 0.  A saturated softmax (z differences of 1e4 and beyond)
 * gives P of exactly 0 and 1 and finite outputs.
 * n == 0 or *n_dev == 0: UNIMM_OK, alive_inv = NaN, group_loss zeroed, no other output is touched.
 * workspace: at least UNIMM_PREF_WS_ITEM_BYTES * (B + groups) bytes, 16-byte aligned, contents irrelevant before and after
 * (fp64 D [B], fp32 c [B], int32 L [B], int32 alive [groups]).
 * UNIMM_E_ARG before any launch: a NULL args or required pointer (ref_rownll and n_dev may be NULL; with n == 0 so may the
 * three arrays of n elements), beta not positive and
 * finite, groups < 1, B < 1, n < 0, a workspace that is too small; UNIMM_E_ALIGN for a workspace off 16-byte alignment. */
#define UNIMM_PREF_MAX_MEMBERS 128
#define UNIMM_PREF_WS_ITEM_BYTES 16
typedef struct {
  const float* rownll;       /* [n] -log p_y of the policy's decoded rows */
  const float* ref_rownll;   /* [n] the same rows under the frozen reference, or NULL */
  const int32_t* row_seq;    /* [n] sequence of each row */
  const int32_t* n_dev;      /* device word: rows actually present (n is then a capacity), or NULL */
  const int32_t* seq_group;  /* [B] */
  const float* seq_weight;   /* [B] */
  float* adv;                /* [n] */
  float* seq_score;          /* [B] */
  float* seq_prob;           /* [B] */
  float* group_loss;         /* [groups] */
  float* alive_inv;          /* [1] */
  void* workspace;
  int64_t workspace_bytes;
  int32_t n, B, groups;
  int32_t length_normalize;  /* 0: D = S - R (val_lm's sum);  else: divided by the row count (val_avg_lm's mean) */
  float beta;
} unimm_seq_pref_args;

int unimm_seq_pref(const unimm_seq_pref_args* args, void* stream);
/* Masked-region KL (models/vilbert_dialog.py:1569-1574): rowloss = [label==1] * sum_j t_j (log t_j - logp_j) */
int unimm_kl_loss_fwd(const float* pred, const float* target, const int32_t* label, float* rowloss, float* lse,
                      int32_t rows, int32_t C, int32_t ld, void* stream);
int unimm_kl_loss_bwd(const float* pred, const float* target, const int32_t* label, const float* lse,
                      const float* g, float inv_denom, void* dpred, int32_t rows, int32_t C, int32_t ld,
                      int32_t ldd, const float* inv_dev, void* stream);
/* Masked-region MSE, the predict_feature = True branch (models/vilbert_dialog.py:1562-1566): rowloss = [label==1] *
 * sum_j (pred_j - target_j)^2 / C (the reference divides the sum over selected ELEMENTS by their count; the caller divides the
 * sum of rowloss by max(#selected rows, 1)).  Backward: dpred = [label==1] g inv_denom 2 (pred - target) / C as bf16 [rows, ldd]
 * (out_split == 0, columns >= C zero) or as an x-type split operand [rows, 3 ldd] (out_split != 0, the fp32-accuracy mode). */
int unimm_mse_loss_fwd(const float* pred, const float* target, const int32_t* label, float* rowloss, int32_t rows, int32_t C,
                       int32_t ld, void* stream);
int unimm_mse_loss_bwd(const float* pred, const float* target, const int32_t* label, const float* g, float inv_denom,
                       void* dpred, int32_t rows, int32_t C, int32_t ld, int32_t ldd, int32_t out_split, void* stream);
/* Weighted 2-way cross-entropy, reduction 'mean' = sum w_y l / sum w_y (models/vilbert_dialog.py:1617-1621);
 * w0, w1 already divided by w0 (:1608). */
int unimm_nsp_loss_fwd(const float* logits, const int32_t* labels, float w0, float w1, float* loss, int32_t B,
                       int32_t ld, void* stream);
/* dlogits: fp32 [B, ldd] (columns 2.. zeroed); extra (or NULL): fp32 [B, 2] added to it -- a gradient that arrives
 * through the returned NSP scores (the ranking loss of dense_annotation_finetuning.py:263-293) */
int unimm_nsp_loss_bwd(const float* logits, const int32_t* labels, float w0, float w1, const float* g, const float* extra,
                       float* dlogits, int32_t B, int32_t ld, int32_t ldd, void* stream);
/* dst[0] = scale * sum(src) (fixed order, deterministic); dst[seg[i]] += sign * src[i].  n_dev (or NULL): only src[0 .. min(n, *n_dev))
 * is read; scale_dev (or NULL): a device word that replaces scale.  segment_sum adds the entries of a segment that follow one
 * another in index order and hands each such run (cut at every 256th entry) to dst with one atomic: segments listed together
 * and no longer than 256 entries -- the per-sequence scores -- come out the same bits in every launch */
int unimm_reduce_sum(const float* src, int64_t n, float* dst, float scale, const int32_t* n_dev, const float* scale_dev,
                     void* stream);
int unimm_segment_sum(const float* src, const int32_t* seg, float* dst, int64_t n, float sign, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused AdamW over the flat arenas.  Replaces the optimizer of train.py:322-347 /
 * :458 (`pytorch_transformers.AdamW`, one parameter group per tensor: lr in {lr, image_lr} by
 * config/language_weights.json, weight_decay in {0.01, 0}); the lr values are whatever the caller's
 * scheduler (utils/optim_utils.py:8-26) set for this step.  Per element, in fp32:
 *   g *= grad_scale;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 *   p -= lr_g * [sqrt(1-b2^step)/(1-b1^step) if correct_bias] * m / (sqrt(v) + eps);  p -= lr_g * wd_g * p
 * group[i] (uint8, device) is the (lr, wd) group of elements [64 i, 64 i + 64); values >=
 * UNIMM_ADAMW_MAX_GROUPS mark parameters that never receive a gradient (skipped entirely, as the
 * reference skips `p.grad is None`).  w16 (bf16, may be NULL) receives the updated parameters: the
 * GEMM-operand copy, so no separate cast pass.  zero_grad != 0 clears g in the same pass. */
#define UNIMM_ADAMW_MAX_GROUPS 8
typedef struct {
  float* p;              /* [n] fp32 parameters (updated in place) */
  float* g;              /* [n] fp32 gradients (cleared in place when zero_grad != 0: not const) */
  float* m;              /* [n] fp32 exp_avg */
  float* v;              /* [n] fp32 exp_avg_sq */
  void* w16;             /* [n] bf16 copy of p or NULL */
  const uint8_t* group;  /* [n / 64] group id per 64-element chunk */
  int64_t n;             /* multiple of 64 */
  int32_t n_groups;      /* <= UNIMM_ADAMW_MAX_GROUPS */
  int32_t step;          /* 1-based step count t */
  double lr[UNIMM_ADAMW_MAX_GROUPS];           /* doubles: the scalar factors (1 - beta, lr * correction,    */
  double weight_decay[UNIMM_ADAMW_MAX_GROUPS]; /* lr * wd) are formed in double and rounded to fp32 once,    */
  double beta1, beta2, eps;                    /* as the reference's Python-float arithmetic does            */
  float grad_scale;      /* 1 / loss scale (or 1 / batch_multiply); 1 = none */
  int32_t correct_bias;
  int32_t zero_grad;
} unimm_adamw_args;

int unimm_adamw_step(const unimm_adamw_args* args, void* stream);

/* Global-norm gradient clipping and a non-finite guard for the step above, without a host sync: a norm pass over the gradient
 * arena leaves its result in a device-resident state block, and unimm_adamw_step_clipped takes its gradient scale from there.
 * The semantics are those of torch.nn.utils.clip_grad_norm_ applied to grad_scale * g (the reference's train.py does not clip;
 * BERT fine-tuning and policy-gradient recipes clip the global norm at about 1).
 *
 * unimm_grad_norm reads g [n] once.  A 64-element chunk COUNTS when group[chunk] < n_groups; ids in [n_groups, 8) (chunks that
 * take no step) and skip ids >= UNIMM_ADAMW_MAX_GROUPS are not read at all, so they may hold any bit pattern, NaN included.
 * Every counted element is widened to fp64 and squared there (a product of two fp32 values is exact in fp64, so a finite gradient
 * of 1e25 gives a finite norm), and every addition is an fp64 addition in a fixed order: per lane over its grid-stride elements,
 * a fixed cross-lane tree, one partial per workgroup and group written to `workspace`, then a second one-workgroup launch that adds
 * the partials in a fixed order (lane t takes workgroups t, t + 256, ... in index order, then the same tree).  No float atomics, no "last block done" counter; the grid is a function of n alone, so the same
 * input gives the same bits on every launch.  One grid-stride pass covers 2048 workgroups x 256 lanes x 2 x 4 = 4,194,304
 * elements; no serial chain of additions is longer than 2 n / 4,194,304 + 48, so with non-negative terms the relative error of
 * sumsq stays below (chain length) x 1.1e-16.
 * The second launch writes the whole state block (fp64 arithmetic):
 *   group_sumsq[k] = sum of g^2 over the chunks of group k (0 for k >= n_groups);   sumsq = group_sumsq[0] + ... in index order
 *   norm      = |grad_scale| * sqrt(sumsq)                 the norm of the gradient the update sees, grad_scale * g
 *   nonfinite = !isfinite(sumsq)                            an inf or NaN in any counted element
 *   coef      = min(1, max_norm / (norm + 1e-6))            max_norm finite;  1 when max_norm is +inf (measure only) or nonfinite
 *   scale     = (float)((double)grad_scale * coef)          grad_scale bit for bit when coef == 1
 *   skipped  += nonfinite                                   a running counter: zero the block once, before its first use
 * workspace: at least UNIMM_GRAD_NORM_WS_DOUBLES doubles, 16-byte aligned, contents irrelevant before and after the call.
 * Refused before any launch: UNIMM_E_ARG for a NULL g, group, workspace or state, n_groups outside 1 .. UNIMM_ADAMW_MAX_GROUPS,
 * a max_norm that is NaN, zero or negative, workspace_doubles < UNIMM_GRAD_NORM_WS_DOUBLES; UNIMM_E_SHAPE for n <= 0 or
 * n % 64 != 0; UNIMM_E_ALIGN for g, workspace or state off 16-byte alignment. */
#define UNIMM_GRAD_NORM_WS_DOUBLES 16384
typedef struct {
  double group_sumsq[UNIMM_ADAMW_MAX_GROUPS];  /* per (lr, wd) group, of the unscaled g */
  double sumsq;
  double norm;
  double coef;
  float scale;           /* what unimm_adamw_step_clipped multiplies every gradient element by */
  int32_t nonfinite;     /* 1 / 0 */
  int32_t skipped;       /* number of norm passes so far that found a non-finite gradient */
} unimm_clip_state;

int unimm_grad_norm(const float* g, const uint8_t* group, int64_t n, int32_t n_groups, float grad_scale, double max_norm,
                    double* workspace, int64_t workspace_doubles, unimm_clip_state* state, void* stream);
/* unimm_adamw_step with the per-element gradient rnd(g * state->scale): the scale is read from device memory and
 * args->grad_scale is IGNORED (it went into unimm_grad_norm).  One kernel template with unimm_adamw_step: with state->scale ==
 * grad_scale bitwise (coef == 1) p, m, v, w16 and g come out bit-equal to unimm_adamw_step's.  skip_nonfinite != 0 and
 * state->nonfinite != 0: every workgroup leaves p, m, v and w16 untouched; zero_grad still clears g on exactly the chunks the
 * update would have cleared (ids < UNIMM_ADAMW_MAX_GROUPS: every counted chunk), or the poison would survive into the next
 * step.  skip_nonfinite == 0: the update runs whatever the flag says, with scale == grad_scale when it is set (coef is 1
 * then); the two options are independent.  Refusals: those of unimm_adamw_step; UNIMM_E_ARG for a NULL state, UNIMM_E_ALIGN
 * for a state off 16-byte alignment. */
int unimm_adamw_step_clipped(const unimm_adamw_args* args, const unimm_clip_state* state, int32_t skip_nonfinite, void* stream);

/* NeuralNDCG-transposed of `slates` independent slates of `n` answer options: value and gradient with
 * respect to the predictions in one launch.  Replaces the deterministic branch of
 * neuralNDCG_transposed (utils/rank_loss.py:518-581: deterministic_neural_sort :79-112, sinkhorn_scaling
 * :55-78, dcg :18-54) as dense_annotation_finetuning.py:286-288 calls it, and its autograd backward.
 * pred / truth fp32 [slates, n]; truth == pad_label marks a padded option.  Outputs per slate:
 * ndcg (0 when the slate has no relevant option), alive (1 / 0: ideal DCG != 0), iters (Sinkhorn sweeps
 * run), and dpred [slates, n] = d ndcg / d pred.  The caller forms loss = -sum(ndcg) / sum(alive). */
#define UNIMM_NDCG_MAX_OPTIONS 128
#define UNIMM_NDCG_MAX_ITER 64
typedef struct {
  const float* pred;
  const float* truth;
  float* ndcg;
  float* alive;
  float* dpred;
  int32_t* iters;
  int32_t slates, n;
  int32_t k;                    /* truncation rank; <= 0 = n */
  int32_t powered_relevancies;  /* gain 2^y - 1 (1) or y (0); the ideal DCG always uses 2^y - 1, as the reference does */
  int32_t max_iter;             /* 1 .. UNIMM_NDCG_MAX_ITER (reference default 50) */
  float pad_label, temperature, tol;
} unimm_ndcg_args;

int unimm_neural_ndcg(const unimm_ndcg_args* args, void* stream);

/* ---------------------------------------------------------------------------------------------
 * fp32-accuracy compute mode ("fp32x3", csrc/x3ops.hip).  The reference's dense-annotation fine-tune calls the model
 * WITHOUT autocast (dense_annotation_finetuning.py:253: fp32 end to end; north_star gates fp32 results at 1e-3).  gfx950
 * has no fast fp32 matrix path, so this mode runs every nn.Linear of the path on the SAME bf16 MFMA kernels
 * (unimm_gemm_nt / unimm_gemm_tn_grouped) over SPLIT operands, x = hi + lo, hi = bf16(x), lo = bf16(x - hi):
 *   activation operand ("x-type")  X3[M, 3 Kp] = [ hi(X) | lo(X) | hi(X) ]
 *   weight operand     ("w-type")  W3[N, 3 Kp] = [ hi(W) | hi(W) | lo(W) ]        Kp = K rounded up to 64, padding zero
 *   unimm_gemm_nt(x = X3, w = W3, K = 3 Kp, out fp32)  =  hi hi + lo hi + hi lo   (fp32 accumulate; lo lo ~ 2^-16 dropped)
 * and a weight gradient as three problems of unimm_gemm_tn_grouped over column planes of two x-type buffers
 * (dY.hi, X.hi), (dY.lo, X.hi), (dY.hi, X.lo), all accumulating into the same fp32 gradient.  Between two GEMMs
 * everything is fp32; the entry points below produce the next split operand from fp32 results, run LayerNorm / loss
 * backward on fp32 gradients, and compute the attention cores (models/vilbert_dialog.py:390-410, :519-539, :681-721)
 * in fp32 on the vector ALUs.
 * ------------------------------------------------------------------------------------------- */
enum { UNIMM_X3_COPY = 0, UNIMM_X3_ADD = 1, UNIMM_X3_GELU = 2, UNIMM_X3_MUL_DGELU = 3 };
typedef struct {
  const float* a;  /* [rows, cols] fp32, row stride lda */
  const float* b;  /* second operand of ADD / MUL_DGELU (row stride ldb) or NULL */
  float* out32;    /* or NULL: y as fp32 [rows, cols], row stride ld32 */
  void* out3;      /* or NULL: y as a split operand, bf16 [rows, 3 cp] (columns cols .. cp-1 of every plane zero) */
  int64_t rows;
  int32_t cols, cp;          /* cp % 64 == 0, cp >= cols */
  int32_t lda, ldb, ld32;
  int32_t op;                /* y = a | a + b | erf-GELU(a) (:115-121) | a * GELU'(b) */
  int32_t wtype;             /* 0: x-type planes (hi, lo, hi); 1: w-type planes (hi, hi, lo) */
} unimm_x3_split_args;
int unimm_x3_split(const unimm_x3_split_args* args, void* stream);
/* transposed w-type split of a weight: src fp32 [R, C] (row stride lds) -> dst bf16 [C, 3 Rp], dst[c][p Rp + r]; columns
 * r in [R, Rp) of every plane are not written (zero-fill dst once).  The operand of the input-gradient GEMMs. */
int unimm_x3_split_wt(const float* src, void* dst, int32_t R, int32_t C, int32_t lds, int32_t Rp, void* stream);
/* unimm_layernorm_bwd_partials on fp32 gradients: dy fp32 [M, H]; dx32 (or NULL) = fp32 gradient w.r.t. the pre-LayerNorm
 * sum; dxd3 (or NULL) = its dropout-masked copy as an x-type split operand [M, 3 H]; partials / blocks_out as there
 * (reduced by unimm_colpartials_finish_grouped).  H % 64 == 0. */
int unimm_x3_layernorm_bwd_partials(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                                    float* dx32, void* dxd3, float* partials, int32_t M, int32_t H, uint32_t drop_key,
                                    uint32_t drop_thr, float drop_scale, uint32_t odrop_key, uint32_t odrop_thr,
                                    float odrop_scale, int32_t* blocks_out, const int32_t* m_dev, const uint32_t* drop_salt,
                                    void* stream);
/* unimm_layernorm_fwd that also writes the normalised rows as an x-type split operand y3 [M, 3 H] (H % 64 == 0); y32 (or NULL),
 * mean / rstd (both or neither), dropout as there. */
int unimm_x3_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y32, void* y3, float* mean, float* rstd,
                           int32_t M, int32_t H, float eps, uint32_t drop_key, uint32_t drop_thr, float drop_scale,
                           const uint32_t* drop_salt, void* stream);
/* unimm_embed_bwd with an fp32 upstream gradient */
int unimm_embed_bwd_f32(const unimm_embed_args* args, const float* dy, float* dword, float* dpos, float* dtype, float* dext,
                        float* dgamma, float* dbeta, float* partials, void* stream);
/* unimm_lm_loss_bwd / unimm_kl_loss_bwd writing x-type split operands [rows, 3 cp] (cp % 64 == 0, cp >= V / C); unlike
 * unimm_lm_loss_bwd, rows of out3 at or past *n_dev (below n) are written as zeros */
int unimm_x3_lm_loss_bwd(const float* logits, const int32_t* labels, const int32_t* weights, const float* lse, const float* g,
                         float inv_denom, void* out3, int32_t n, int32_t V, int32_t ld, int32_t cp, const int32_t* n_dev,
                         const float* inv_dev, void* stream);
int unimm_x3_kl_loss_bwd(const float* pred, const float* target, const int32_t* label, const float* lse, const float* g,
                         float inv_denom, void* out3, int32_t rows, int32_t C, int32_t ld, int32_t cp, const float* inv_dev,
                         void* stream);
/* dst[idx[r], :] += src[r, :], both fp32 (unimm_rows_add_f32 for an fp32 gradient stream) */
int unimm_x3_rows_add(float* dst, const int32_t* idx, const float* src, int32_t n, int32_t H, int32_t ldd, void* stream);
/* unimm_attn_fwd / unimm_attn_bwd with fp32 q / k / v / out / dout / dq / dk / dv (same argument structs, row strides in
 * fp32 elements, multiples of 4; every other field -- masks, lse, variable-length offsets, dropout -- as there). */
typedef struct {
  void* out3;                      /* forward: the context ALSO as an x-type split operand [rows, 3 cp3] (bf16), or NULL */
  void* dq3; void* dk3; void* dv3; /* backward: dQ / dK / dV as x-type split operands INSTEAD of fp32 (all three or none; the args'
                                    * dq / dk / dv may then be NULL); each points at its first column of plane 0 */
  int32_t ld3;                     /* row stride of the split buffers, bf16 elements (>= 3 cp3) */
  int32_t cp3;                     /* plane stride = columns per plane (multiple of 8, >= H * D); buffers 16-byte aligned, ld3 % 8 == 0 */
} unimm_x3_attn_planes;
/* planes (or NULL): what the next GEMM reads, written by the attention kernel itself instead of a unimm_x3_split pass over its
 * fp32 result.  Matrix-instruction kernels only (UNIMM_E_ARG under unimm_x3_attn_set_impl(0)).
 * unimm_x3_attn_fwd takes the spliced shared key/value segment (ks_off / ks_len / ks_ins of the argument struct, same meaning
 * and same checks as in unimm_attn_fwd) in its matrix-instruction kernels: out, lse and the split planes are bit-identical to a
 * launch over the same rows gathered into position order.  UNIMM_E_ARG under unimm_x3_attn_set_impl(0); unimm_x3_attn_bwd
 * has no way to pass one. */
int unimm_x3_attn_fwd(const unimm_attn_args* args, const unimm_x3_attn_planes* planes, void* stream);
int unimm_x3_attn_bwd(const unimm_attn_bwd_args* args, const unimm_x3_attn_planes* planes, void* stream);
/* Which kernels the two entry points above launch: 1 (default) = the fp32 matrix-instruction kernels
 * (v_mfma_f32_16x16x4_f32, exact fp32 operands), 0 = the vector-ALU kernels of the first version (kept for A/B runs). */
int unimm_x3_attn_set_impl(int32_t impl);

/* ---------------------------------------------------------------------------------------------
 * Answer generation (unimm_amd/generation.py; ABI 19, sampling ABI 20).  Under the generative mask (utils/data_utils.py:199-210) the context
 * rows [1, c) and the image stream never see the answer, answer row c+k attends [1, c+k] and the [MASK]-copy row of answer
 * token k attends [1, c+k) + itself: the sequence is a prefix-LM, so a decode step pushes only the NEW text rows of every
 * hypothesis through the blocks and reads everything older from a key/value cache.
 * ------------------------------------------------------------------------------------------- */
/* Text self-attention (models/vilbert_dialog.py:390-410) of the new rows of G groups x `beams` hypothesis slots, D = 64,
 * H * D <= 1024.  Hypothesis slot s = g * beams + b owns the new rows [s * nr, s * nr + nr) of q / k / v / out (nr = 1 or 2:
 * answer row k-1, then copy row k).  New row i of slot s attends, in this order: the group's SHARED context rows
 * [ctx_off[g], ctx_off[g] + ctx_len[g]) of ctx_k / ctx_v, the slot's PRIVATE cached answer rows [0, plen[s]) (row r at
 * priv_k / priv_v + (s * pcap + r) * ldp), and its own new rows [0, i] (k / v of the same call).  That is exactly the
 * generative mask: a masked key's exp(-10000 + s) underflows to 0 in fp32 in the reference, so no mask words are read.
 * One workgroup per (group, head) takes all nr * beams <= 32 query rows, so the context K / V of a group is read once;
 * K / V rows go straight to VGPRs (kernel guide: attention decode / GEMV, M <= 16), dot products and P.V on the vector ALU
 * in fp32.  No split over keys: one head's context is at most 255 x 64 x 2 x 2 B = 65 KB, microseconds at one CU's bandwidth
 * (revisit if a profile disagrees; measured at 80 dialogs x 4 beams: ~69 us per launch, second to the NT GEMMs in a decode step --
 * a matrix-instruction form of the score and P.V products is the next step).  ctx_len[g] <= 256 and ctx_len[g] + plen[s] + nr <= 320; out is written in the layout of unimm_attn_fwd
 * (row, head * 64 + d).  Row strides in elements, multiples of 8; every pointer 16-byte aligned.
 * Values outside those bounds are clamped, never followed out of the buffers: ctx_len[g] is taken as min(max(ctx_len[g], 0), 256),
 * and plen[s] as min(max(plen[s], 0), pcap, 320 - nr - ctx_len[g]) -- a negative plen is 0, plen > pcap is pcap, and with
 * ctx_len = 256, nr = 2 a slot sees its first 62 private rows whatever pcap is.  Nothing else is read: not the rows between the
 * groups' contexts, not the private rows at and past the clamped plen[s], not a column outside [0, H * 64) of any row; of `out`
 * exactly the columns [0, H * 64) of the G * beams * nr rows are written.  ctx_len[g] = 0 is allowed (a row then attends the
 * private and new rows only); ctx_off need not be ascending. */
typedef struct {
  const void* q; const void* k; const void* v;   /* bf16, the new rows' fused projection (row strides ldq / ldk / ldv) */
  void* out;                                     /* bf16 [G * beams * nr, ldo] */
  const void* ctx_k; const void* ctx_v;          /* bf16 shared context rows, row stride ldc */
  const int32_t* ctx_off; const int32_t* ctx_len; /* int32 [G], device */
  const void* priv_k; const void* priv_v;        /* bf16 private caches [G * beams][pcap] rows, row stride ldp (or NULL when pcap = 0) */
  const int32_t* plen;                           /* int32 [G * beams], device: cached answer rows of each slot (<= pcap) */
  int32_t G, beams, nr, H, D, pcap;
  int32_t ldq, ldk, ldv, ldo, ldc, ldp;
  float scale;
} unimm_attn_decode_args;
int unimm_attn_decode(const unimm_attn_decode_args* args, void* stream);

/* Per-step maintenance of the private caches of all `layers` text layers in one launch, after beam selection:
 * for every slot s with parent p = parent[s] (a slot of the previous step), dst rows [0, plen[p]) of s = src rows of p, and dst
 * row plen[p] of s = p's new answer row: new_kv + layer * new_layer_stride + (p * new_row_mul) * ld_new (width elements, the K
 * and V columns of one layer are `width` contiguous elements, e.g. K | V of the fused projection); plen_out[s] = plen[p] + 1.
 * Cache layout: src / dst + ((layer * slots + s) * pcap + r) * ldp, width <= ldp.  src and dst must not overlap (the
 * reorder is a gather); bit-exact copies.  plen[p] + 1 <= pcap, width % 8 == 0, strides % 8 == 0.
 * Clamps: parent[s] is taken as min(max(parent[s], 0), slots - 1) and plen[p] as min(max(plen[p], 0), pcap - 1), so a full
 * parent (plen[p] = pcap) keeps its first pcap - 1 rows, gets the new row as its last and reports plen_out = pcap.  Of dst
 * exactly the columns [0, width) of the rows [0, plen_out[s]) of every slot are written; columns past `width` of src and of the
 * new rows are not read.  src == dst or plen == plen_out returns UNIMM_E_ARG, a misaligned pointer / width / stride
 * UNIMM_E_ALIGN, both before any launch. */
typedef struct {
  const void* src; void* dst;                    /* bf16 [layers][slots][pcap][ldp] */
  const void* new_kv;                            /* bf16 */
  const int32_t* parent; const int32_t* plen; int32_t* plen_out;   /* int32 [slots], device */
  int32_t layers, slots, pcap, ldp, width;
  int64_t new_layer_stride;                      /* elements */
  int32_t ld_new, new_row_mul;
} unimm_kv_update_args;
int unimm_kv_cache_update(const unimm_kv_update_args* args, void* stream);

/* Speculative decoding (unimm_amd/speculative.py).  The pair-structured form of unimm_attn_decode: the nr new rows of a slot are
 * nr / 2 (answer row, copy row) pairs that go through the blocks at once; new row i of a slot is pair i / 2, kind i % 2 (0 = answer
 * row, 1 = copy row).  Every new row attends, in this order: the group's shared context rows, the slot's private rows [0, plen[s]),
 * the new ANSWER rows (even rows) of the pairs <= its own pair, in pair order, and -- a copy row -- itself.  No row attends another
 * copy row or an answer row of a later pair: with answer rows n-1 .. and copy rows n .. of consecutive steps that is the generative
 * mask of every one of those steps.  Same struct, same layout of every buffer, same clamps (ctx_len[g] to [0, 256], plen[s] to
 * [0, min(pcap, 320 - nr - ctx_len[g])]: with ctx_len = 256, nr = 32 a slot sees its first 32 private rows) and the same statement
 * of what is read and written as unimm_attn_decode; fp32 scores and P.V on the vector ALU in that kernel's order of operations.
 * nr even, 2 <= nr <= 32, beams * nr <= 32, D = 64, anything else UNIMM_E_SHAPE before a launch.  nr = 2 is unimm_attn_decode's
 * rule, and `out` is bit-identical to its. */
int unimm_attn_verify(const unimm_attn_decode_args* args, void* stream);

/* In-place append to the private caches of all `layers` text layers in one launch; the slots keep their parents.  Slot s copies
 * count[s] new rows into cache rows plen[s] .. plen[s] + count[s] - 1 of every layer: source row j is
 * new_kv + layer * new_layer_stride + (s * new_row_mul + j * new_row_step) * ld_new (width elements), destination
 * cache + ((layer * slots + s) * pcap + plen[s] + j) * ldp; plen_out[s] = plen[s] + count[s].  Bit-exact copies.
 * Clamps: plen[s] is taken as min(max(plen[s], 0), pcap), count[s] as min(max(count[s], 0), max_count, pcap - plen[s]): a full
 * slot appends nothing and reports plen_out = pcap.  Of the cache exactly the columns [0, width) of the named rows are written;
 * of the new rows only those columns of the count[s] named rows are read.  width % 8 == 0, strides % 8 == 0, width <= ldp.
 * plen == plen_out returns UNIMM_E_ARG (every layer's workgroup reads plen[s] while one of them writes plen_out[s]), a
 * misaligned pointer / width / stride UNIMM_E_ALIGN, both before any launch. */
typedef struct {
  void* cache;                                   /* bf16 [layers][slots][pcap][ldp] */
  const void* new_kv;                            /* bf16 */
  const int32_t* count; const int32_t* plen; int32_t* plen_out;    /* int32 [slots], device */
  int32_t layers, slots, pcap, ldp, width, max_count;
  int64_t new_layer_stride;                      /* elements */
  int32_t ld_new, new_row_mul, new_row_step;
} unimm_kv_append_args;
int unimm_kv_cache_append(const unimm_kv_append_args* args, void* stream);

/* Log-softmax + top-K of fp32 logits [rows, ldl] (models/vilbert_dialog.py:1023-1026 decoder output), one row per
 * workgroup, the vocabulary streamed once with an online log-sum-exp.  logp = logit - lse over ALL V ids (no renormalisation
 * after banning).  Then -inf for: the `nbanned` ids of `banned` (int32, device), id `sep` when flags[row] & 1, every id other
 * than `sep` when flags[row] & 2 (flags int32 [rows] or NULL).  Returns the K <= 16 largest (vals fp32 [rows, K], ids int32
 * [rows, K]) ordered by (value desc, id asc) -- -inf entries included, by the same rule; lse fp32 [rows] or NULL.
 * The order is decided on the raw fp32 logits (exact ties by id), not on the rounded logp.  V <= 65536, K <= V, ldl >= V (no
 * alignment asked of ldl); columns past V are not read.  Banned ids outside [0, V) and duplicates are ignored, `banned` may be
 * NULL when nbanned = 0, and nbanned is not bounded by the block size.  -inf logits are candidates like any other (they add
 * nothing to lse and rank last, by id); a row whose logits are ALL -inf has lse = -inf and NaN values.  rows = 0 returns
 * UNIMM_OK without a launch and leaves the outputs untouched. */
int unimm_lm_topk(const float* logits, int32_t rows, int32_t V, int32_t ldl, const int32_t* banned, int32_t nbanned,
                  const int32_t* flags, int32_t sep, int32_t K, float* vals, int32_t* ids, float* lse, void* stream);

/* Sampling from fp32 logits [rows, ldl] (ABI 20): temperature, top-k and nucleus filtering and one draw per row, one workgroup
 * per row; logits / V / ldl / banned / nbanned / flags / sep as in unimm_lm_topk.  Per row, in this order:
 *  1. ELIGIBLE ids: [0, V) without the banned ids, without `sep` when flags[row] & 1, without every id other than `sep` when
 *     flags[row] & 2 (with a finite logit of `sep` that row returns token = sep, logq = 0 whatever the other arguments are),
 *     and without the ids whose logit is not > -inf.  Nothing eligible: token = -1, logp = logq = -inf (lse is still written).
 *  2. RANK by (raw fp32 logit desc, id asc), the order of unimm_lm_topk (-0 ties +0).  top_k > 0 keeps exactly the first
 *     min(top_k, #eligible) ids of that order (an exact radix select on the order-preserving integer image of the fp32 bits, a
 *     second one on the id among the logits tied at the boundary); top_k = 0 keeps all, and top_k is not bounded by 16.
 *  3. TEMPERATURE: y_i = x_i / temperature, q_i ~ exp(y_i - max y) over the kept ids; the kernel evaluates y_i - max y as
 *     (x_i - x_max) / temperature, so that its rounding does not grow with an offset common to the row.
 *  4. NUCLEUS, top_p < 1: keep {i : x_i >= theta}, theta the largest logit of the row whose mass sum{q_i : x_i >= theta} is
 *     >= top_p * sum q.  Ids tied with theta all stay; the top-ranked id always stays.  Masses are summed in 2^-40 fixed point
 *     (q_i <= 1) in 64-bit integers, whose sum does not depend on the order of the additions; the comparison is
 *     mass >= ceil((double)top_p * (double)total) in those units.
 *  5. DRAW by Gumbel-max: token = argmax over the kept ids of y_i + g_i (ties to the smaller id), g_i = -log(-log u_i),
 *     u_i = ((h_i >> 9) + 0.5) * 2^-23 (exact in fp32, inside (0, 1)),
 *     h_i = mix32(mix32(key ^ (stream_ids[row] * 0x9E3779B1 + 0x7F4A7C15)) + i * 0x85EBCA77), mix32 the hash of csrc/common.h
 *     (host mirror: unimm_amd/dropout.py mix32_int); logf is the accurate one.  A draw depends on (key, stream_ids[row], the
 *     row's logits and flags) alone: not on the row's position, the number of rows or an earlier launch.
 *  6. logq[row] = y_t - logsumexp over the kept ids of y: the log-probability under the distribution sampled from.
 * logp[row] = x_t - logsumexp(x[0:V]), the value unimm_lm_topk reports for that id (the same online log-sum-exp), lse fp32 [rows]
 * or NULL.  token int32 [rows], logp / logq fp32 [rows], stream_ids int32 [rows] (device).
 * Which path a V takes: V <= 36864 stages the row's keys once in LDS (4 V bytes of dynamic LDS: 119 KiB at V = 30522) and runs
 * every selection pass over LDS; a larger V (<= 65536) re-reads the L2-resident row in every pass.  Same results either way.
 * V <= 65536, ldl >= V, columns past V are not read; banned ids outside [0, V) and duplicates are ignored; rows = 0 returns
 * UNIMM_OK without a launch and leaves the outputs untouched.  temperature <= 0 (or not finite), top_p outside (0, 1] and
 * top_k < 0 return UNIMM_E_ARG before any launch. */
int unimm_lm_sample(const float* logits, int32_t rows, int32_t V, int32_t ldl, const int32_t* banned, int32_t nbanned,
                    const int32_t* flags, int32_t sep, float temperature, int32_t top_k, float top_p, uint32_t key,
                    const int32_t* stream_ids, int32_t* token, float* logp, float* logq, float* lse, void* stream);

/* The same with PER-ROW decoding parameters (ABI 24): temperature fp32 [rows], top_k int32 [rows] and top_p fp32 [rows] are
 * device arrays, everything else is unimm_lm_sample's (the same kernel template; both the LDS-staged and the re-read path).
 * Row r is processed exactly as unimm_lm_sample processes it when launched with (temperature[r], top_k[r], top_p[r]): steps 1-6,
 * logp, logq and lse are bit-identical, and a row depends on its own logits, flags, stream id and parameters alone -- not on
 * its position, on the other rows or on their parameters.  So one launch can mix decoding rules, and:
 *  - a row with top_k = 1 is GREEDY: token = the first id of the rank order of step 2 (the id unimm_lm_topk reports first),
 *    logp = the value unimm_lm_topk reports for it, logq = 0 exactly, whatever its temperature, top_p and stream id are;
 *  - the host cannot see the values, so the kernel refuses them per row: a row whose temperature is not positive and finite,
 *    whose top_p is outside (0, 1] or whose top_k < 0 returns token = -1, logp = logq = -inf (lse is still written, and
 *    nothing is read out of bounds); the other rows of the launch are not affected.
 * Any of the three arrays NULL returns UNIMM_E_ARG before any launch (as do the NULL cases of unimm_lm_sample); rows = 0
 * returns UNIMM_OK without a launch and leaves the outputs untouched. */
int unimm_lm_sample_rows(const float* logits, int32_t rows, int32_t V, int32_t ldl, const int32_t* banned, int32_t nbanned,
                         const int32_t* flags, int32_t sep, const float* temperature, const int32_t* top_k, const float* top_p,
                         uint32_t key, const int32_t* stream_ids, int32_t* token, float* logp, float* logq, float* lse,
                         void* stream);

/* A per-row token HISTORY for unimm_lm_topk_hist / unimm_lm_sample_hist: what each row's hypothesis has already said, and the
 * two rules that depend on it (generate_answers' no_repeat_ngram_size / repetition_penalty / repeat_scope).  Row r has the
 * SOURCES  a = hist[r, 0:k), k = hist_len[r] clamped to [0, ldh]  (its answer tokens), and, when ctx is not NULL,
 * s = ctx[i, 0:ctx_len[i]), i = ctx_idx[r] clamped to [0, nctx), the length clamped to [0, ldc]  (its dialog's context tokens).
 *  - N-GRAM rule, ngram = n in [1, 8] (0 = off): when k >= n - 1, id t is banned for the row if some source s and some end
 *    e >= n - 1 have s[e-n+1 .. e) == a[k-n+1 .. k) and s[e] == t.  A window lies inside ONE source; overlapping windows count
 *    (n = 2 after `a a` bans a); n = 1 bans every id of the sources; k < n - 1 bans nothing from either source.  `sep` (this
 *    struct's) is never banned by the rule; source ids outside [0, V) ban nothing but compare as integers.  Such a ban acts
 *    exactly like an id of `banned`: -inf after the log-sum-exp, no renormalisation, out of the eligible set of step 1.
 *  - PENALTY rule, penalty = r != 1: every id i that occurs in a source is SELECTED by x'_i = x_i > 0 ? x_i * inv_penalty :
 *    x_i * penalty -- one correctly rounded fp32 product, rounded before anything is subtracted from it -- and every other id by
 *    x_i.  The rank order, top-k, y, q, nucleus, draw and logq of unimm_lm_sample's steps 2-6 are those of the row x'; lse and
 *    logp are those of the raw row x.  unimm_lm_topk_hist orders its K ids by x' and reports x_i - lse for each.
 *    inv_penalty is the caller's fp32 1 / r (a product, not a division, so a caller can reproduce x' bit for bit).
 * Refused before any launch: a NULL struct, penalty or inv_penalty not positive and finite, hist NULL with ngram > 0 or
 * penalty != 1, hist without hist_len, ctx without ctx_len or ctx_idx (UNIMM_E_ARG); ngram outside [0, 8], ldh outside
 * [0, 128], ldc outside [0, 256], nctx < 1 with a ctx (UNIMM_E_SHAPE).  With ngram = 0 and penalty = 1 nothing of the
 * history is used and the launch computes what the plain entry point computes. */
typedef struct {
  const int32_t* hist; const int32_t* hist_len;  /* int32 [rows, ldh], int32 [rows], device */
  const int32_t* ctx; const int32_t* ctx_len; const int32_t* ctx_idx;   /* int32 [nctx, ldc], [nctx], [rows], device; or NULL */
  int32_t ldh, nctx, ldc;
  int32_t ngram, sep;
  float penalty, inv_penalty;
} unimm_lm_history;

/* unimm_lm_topk with a history (the same kernel template): the bans of the n-gram rule join those of `banned` and the flags,
 * and under a penalty the K ids come in the order of x' with vals = x - lse (a banned id keeps -inf).  Everything else, the
 * refusals included, is unimm_lm_topk's; with ngram = 0 and penalty = 1 the outputs are bit-identical to it.  A row depends on
 * its own logits, flags and history alone. */
int unimm_lm_topk_hist(const float* logits, int32_t rows, int32_t V, int32_t ldl, const int32_t* banned, int32_t nbanned,
                       const int32_t* flags, int32_t sep, int32_t K, const unimm_lm_history* history, float* vals, int32_t* ids,
                       float* lse, void* stream);

/* unimm_lm_sample_rows with a history (the same kernel template, per-row temperature / top_k / top_p).  With penalty = 1 row r
 * is bit-identical to unimm_lm_sample_rows on that row with the rule's bans added to `banned`; with a penalty token and logq
 * are those of unimm_lm_sample_rows on the row x', lse that of the raw row and logp = x_token - lse.  The second bitmap costs LDS:
 * this entry point stages the keys for V <= 34816 (136 KiB of keys + 21.6 KiB of static LDS <= 160 KiB; V = 30522 is staged)
 * and re-reads the row in every pass above that.  Same results either way. */
int unimm_lm_sample_hist(const float* logits, int32_t rows, int32_t V, int32_t ldl, const int32_t* banned, int32_t nbanned,
                         const int32_t* flags, int32_t sep, const float* temperature, const int32_t* top_k, const float* top_p,
                         uint32_t key, const int32_t* stream_ids, const unimm_lm_history* history, int32_t* token, float* logp,
                         float* logq, float* lse, void* stream);

/* The rejection step of SPECULATIVE SAMPLING (unimm_amd/speculative.py): one workgroup per row, a row = the model's logits x
 * [rows, ldl], the draft's logits xd [rows, ldd] for the same position, and the token d = draft_token[row] the draft drew there
 * (-1: the row has no draft).  banned / nbanned / flags / sep / V / stream_ids and the per-row temperature / top_k / top_p
 * arrays are unimm_lm_sample_rows' and apply to BOTH rows.  Per row, in this order:
 *  1. P~ is the distribution unimm_lm_sample_rows draws from on the row x with the row's parameters: steps 1-4 of
 *     unimm_lm_sample (the eligible ids, the rank order, exact top-k with the id tie-break, y_i = (x_i - x_max) / t, the nucleus
 *     with its fixed-point masses).  K_P is its kept set, log P~_i = y_i - logsumexp_{K_P} y (the sampler's logq of id i).
 *  2. Q~, K_Q and log Q~_i are the same construction on the row xd: the same banned ids, flags and parameters, xd's own
 *     finiteness test.  Nothing eligible in xd: K_Q is empty.
 *  3. A row whose temperature is not positive and finite, whose top_p is outside (0, 1] or whose top_k < 0 returns token = -1,
 *     accept = 0, logp = logq = log_ratio = -inf (lse is still written): the rule of unimm_lm_sample_rows.
 *  4. Nothing eligible in x: the same result, lse still written.
 *  5. A forced-sep row (flags & 2 with a finite x_sep) has K_P = {sep}, so the steps below give token = sep, logq = 0 and
 *     accept = (d == sep).
 *  6. RATIO  a = log P~_d - log Q~_d when d is in K_P and in K_Q; +inf when d is in K_P and not in K_Q; -inf when d is outside
 *     [0, V) or outside K_P.  log_ratio[row] = a (log_ratio may be NULL).
 *  7. ACCEPT iff logf(u) < a, u = ((h >> 9) + 0.5) * 2^-23 with h the sampler's h_0 of (key_accept, stream_ids[row]), i.e.
 *     mix32(mix32(key_accept ^ (stream_ids[row] * 0x9E3779B1 + 0x7F4A7C15))).  On accept token = d.
 *  8. RESIDUAL on reject: rho_i = exp(log Q~_i - log P~_i) on the ids of K_P that are in K_Q, 0 on the others of K_P; the
 *     candidates are the ids of K_P with rho_i < 1; token = argmax over them of (y_i + log1p(-rho_i)) + g_i (ties to the smaller
 *     id), g_i the sampler's Gumbel noise of (key_residual, stream_ids[row], i): Gumbel-max on log(P~_i - Q~_i) with the row
 *     constant dropped, i.e. a draw from the normalised max(0, P~ - Q~).  No candidate (rounding, or P~ <= Q~ on all of K_P):
 *     token = the first id of P~'s rank order.
 *  9. logp = x_token - logsumexp(x[0:V]) (the sampler's value; lse likewise), logq = log P~_token: the emitted token of an
 *     accept-or-residual step is distributed as P~, so this is the log-probability under the distribution sampled from.
 * Met bit for bit: (i) a row with d = -1 returns the token, logp, logq and lse of unimm_lm_sample_rows launched with
 * key = key_residual (accept = 0, log_ratio = -inf); (ii) with xd the same buffer as x and d in K_P, log_ratio = 0 exactly and
 * accept = 1; (iii) a row with top_k = 1 returns the first id unimm_lm_topk reports, logq = 0 and accept = (d == that id),
 * whatever the keys are; (iv) a row depends on its own inputs alone -- not on its position, the number of rows or an earlier
 * launch.  The same inputs give the same bits (integer masses, no float atomics).
 * How Q~ reaches the kernel: the kernel itself runs the sampler's selection on xd first (keys staged in LDS for V <= 36864),
 * keeps K_Q as a descriptor in registers -- the top-k key and id cut, the nucleus key, xd_max and the log of the kept mass, from
 * which membership and log Q~_i follow from (xd_i, i) alone -- then runs the selection on x over the same LDS and makes one pass
 * over K_P that reads xd_i from memory against the descriptor.  Traffic per row: x once, xd twice (a row with d = -1: x only);
 * V > 36864 re-reads the L2-resident rows in every pass, as the sampler does.  Same results either way.
 * V <= 65536, ldl >= V, ldd >= V, columns past V are not read; flags, banned (with nbanned = 0) and log_ratio may be NULL, any
 * other NULL array returns UNIMM_E_ARG before any launch; rows = 0 returns UNIMM_OK without a launch and leaves the outputs
 * untouched. */
typedef struct {
  const float* x; const float* xd;               /* fp32 [rows, ldl], fp32 [rows, ldd], device */
  const int32_t* draft_token;                    /* int32 [rows] */
  const int32_t* banned; const int32_t* flags; const int32_t* stream_ids;
  const float* temperature; const int32_t* top_k; const float* top_p;   /* [rows] each */
  int32_t* accept; int32_t* token;               /* int32 [rows] */
  float* logp; float* logq; float* lse; float* log_ratio;               /* fp32 [rows]; log_ratio or NULL */
  int32_t rows, V, ldl, ldd, nbanned, sep;
  uint32_t key_accept, key_residual;
} unimm_lm_spec_verify_args;
int unimm_lm_spec_verify(const unimm_lm_spec_verify_args* args, void* stream);

/* Launch profiler for bench.py's `roofline` block: HIP events around every GEMM launch on its own
 * stream while enabled.  Variant index: 0..11 = unimm_gemm_nt (epilogue * 2 + out_f32), 12 = unimm_gemm_tn.
 * unimm_prof_collect synchronises the events and returns per-variant summed milliseconds, algorithmic
 * FLOPs (2*M*N*K per launch) and launch counts; arrays of >= 20 entries.  on = 1: every GEMM launch;
 * on = 2: unimm_gemm_tn launches only (the two event records per launch are host time, which a
 * launch-rate-bound step should not pay for all ~340 GEMM launches); 0 = off. */
int unimm_prof_enable(int32_t on);
int unimm_prof_collect(double* ms, double* flops, int32_t* count, int32_t nvar);
/* Caller-side tag (0 .. 7, default 0) carried by the unimm_gemm_nt launches that follow; unimm_prof_tagged returns, per tag, the
 * summed milliseconds / FLOPs / launch counts of the records the LAST unimm_prof_collect consumed.  The engine tags the launches
 * it issues from inside a BertConnectionLayer (models/vilbert_dialog.py:655-783) with 1: bench.py's
 * `roofline.coattention_gemms`, the figure north_star's ">= 40 % MFMA utilisation on the co-attention GEMMs" is judged by. */
int unimm_prof_tag(int32_t tag);
/* union_ms (or NULL): per tag > 0, the length of the UNION of the launches' execution intervals on one time axis -- launches
 * of two streams that ran side by side count once: the wall time during which at least one tagged GEMM was executing. */
int unimm_prof_tagged(double* ms, double* flops, int32_t* count, double* union_ms, int32_t ntags);

#ifdef __cplusplus
}
#endif
#endif /* UNIMM_HIP_H */
