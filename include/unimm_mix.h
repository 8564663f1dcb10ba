/* unimm_mix.h -- C ABI of libunimm_mix.so, the extension library of libunimm_hip.so (unimm_hip.h) for ensemble and contrastive
 * answer generation: one hand-written gfx950 (MI355X) kernel, built from unimm_amd/csrc/mix/ by unimm_amd/build.py next to the
 * main library and bound by unimm_amd/mix.py.  It is a library of its own so that the main library, its ABI (unimm_version) and its
 * kernels are exactly what they are without it; tests/golden/kernel_resources_mix.json holds its kernel's registers, scratch and LDS.
 *
 * The reference (ZihaoW123/UniMM) ensembles by averaging the SCORES of five checkpoints on the host (evaluate.py:107-118); an
 * ensemble that writes an answer has to mix the members' next-token distributions at every step, which is what this entry point
 * does on the device. */
#ifndef UNIMM_MIX_H
#define UNIMM_MIX_H

#include "unimm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int unimm_mix_version(void);      /* ABI version of this library, bumped on any signature change */

/* MIX the next-token distributions of K = 1 .. 5 models (ensemble and contrastive answer generation, unimm_amd/generation.py):
 * one workgroup per row; member m's fp32 logits row is x[m] + row * ld[m] (ld[m] >= V; no alignment is asked of a base or a
 * stride), the mixed row is out + row * ldo.  Columns at or past V are neither read nor written.  unimm_lm_topk, unimm_lm_sample,
 * _rows and _hist then run on `out` unchanged: they take their log-sum-exp over all V ids and -inf entries add nothing to it, so
 * their log p is the log-probability under the normalised mixture (with a cut: normalised over the plausible set).
 *  mode UNIMM_MIX_LOGIT (log-linear mixture, weights of any sign): z_i = w[0] * x_0,i, then z_i = z_i + w[m] * x_m,i for m = 1 ..
 *   K-1 in order, every product and every sum rounded to fp32 on its own (no fused multiply-add): a numpy float32 restatement is
 *   equal bit for bit.  softmax(z) is the normalised product of the members' distributions raised to w[m], so no log-sum-exp is
 *   taken.  The inputs must be finite (not checked).
 *  mode UNIMM_MIX_PROB (arithmetic mixture, the usual ensemble): z_i = log sum_m w[m] exp(x_m,i - lse_m), lse_m the log-sum-exp
 *   of member m's row over all V ids, evaluated as t_m = (x_m,i - lse_m) + logf(w[m]), z_i = T + logf(sum_m expf(t_m - T)) with
 *   T = max_m t_m, m ascending; members with w[m] == 0 are skipped (their rows are not read).  A -inf entry is probability 0
 *   (t_m = -inf); when every contributing member is -inf at an id, z_i = -inf.  +inf and NaN entries are not supported.  The row
 *   sums to 1, so a selection kernel's lse of it is 0 up to rounding.  How lse_m is summed (per thread, wave, workgroup) is
 *   stated at the top of csrc/mix/lm_mix.hip; it differs between the 16-byte and the scalar path in the order of the sum alone.
 *  PLAUSIBILITY CUT (log_alpha > -inf; -inf = off): m0 = the largest x_0,i of member 0's RAW row over the eligible ids -- i < V,
 *   not in banned[0:nbanned] (ids outside [0, V) ban nothing), not sep when flags[row] & 1 (flags may be NULL) -- and b the
 *   smallest id that reaches it.  Every id i != sep, i != b with x_0,i < m0 + log_alpha (one fp32 add, one compare) gets
 *   out_i = -inf; every other id out_i = z_i: the cut and the mixing are independent.  sep is never cut (a forced end keeps its
 *   id) and neither is b (a row keeps an eligible id); a row without an eligible id is not cut at all.
 * Traffic: LOGIT without a cut reads every row once; with a cut member 0's row twice; PROB every contributing row twice.  Rows
 * are read and written 16 bytes at a time when every base is 16-byte aligned and every stride a multiple of 4, one float at a
 * time otherwise; the results of LOGIT and of the cut do not depend on which.
 * UNIMM_E_ARG before any launch: args or out NULL, K outside [1, 5], an unknown mode, rows < 0, V outside [1, 65536], ldo < V or
 * any ld[m] < V, nbanned < 0 or banned NULL with nbanned > 0, x[m] NULL or w[m] not finite for an m < K, in PROB mode a negative
 * weight or all weights zero, and `out` overlapping a member (the bounding ranges [base, base + (rows - 1) * ld + V) compared).
 * rows = 0 returns UNIMM_OK without a launch.  `stream` is a hipStream_t passed as void*, pointers are device pointers and the
 * call only enqueues work: the conventions of unimm_hip.h, whose UNIMM_* result codes it returns. */
#define UNIMM_MIX_MAX_MEMBERS 5
enum { UNIMM_MIX_LOGIT = 0, UNIMM_MIX_PROB = 1 };
typedef struct {
  const float* x[UNIMM_MIX_MAX_MEMBERS];         /* fp32 [rows, ld[m]] each, device; entries at or past K are ignored */
  float* out;                                    /* fp32 [rows, ldo] */
  const int32_t* banned; const int32_t* flags;   /* int32 [nbanned] or NULL; int32 [rows] or NULL: the cut reads them */
  int32_t ld[UNIMM_MIX_MAX_MEMBERS];
  float w[UNIMM_MIX_MAX_MEMBERS];
  int32_t K, mode, rows, V, ldo, nbanned, sep;
  float log_alpha;
} unimm_lm_mix_args;
int unimm_lm_mix(const unimm_lm_mix_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIMM_MIX_H */
