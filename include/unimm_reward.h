/* unimm_reward.h -- C ABI of libunimm_reward.so, the extension library of libunimm_hip.so (unimm_hip.h) for the consensus reward of
 * self-critical answer training and of generation metrics: one hand-written gfx950 (MI355X) kernel, built from
 * unimm_amd/csrc/reward/ by unimm_amd/build.py next to the main library and bound by unimm_amd/reward_abi.py (the Python surface
 * is unimm_amd/reward.py).  It is a library of its own so that the main library, its ABI (unimm_version) and its kernels are
 * exactly what they are without it; tests/golden/kernel_resources_reward.json holds its kernel's registers, scratch and LDS.
 *
 * THE DEFINITION (CIDEr-D, Vedantam et al. 2015, as self-critical sequence training uses it; tests/reward_ref.py restates it in
 * float64 Python and everything else refers to this text).  Parity with a CIDEr library is unpinned: none was at hand.
 *  Answers.  An answer is a row of token ids >= 0 "tokens, then [SEP], zero padded" with a length that counts the [SEP]; length
 *   <= 0 means absent.  Its effective length is L = len - 1: the [SEP] and everything after it are never read.  For n = 1 .. 4
 *   the n-grams of an answer are its max(0, L - n + 1) windows of n tokens; tf(x) is how often window x occurs in the answer.
 *  Document frequencies.  idf(x) = log(D) - log(max(1, df(x))), D the number of corpus answers and df(x) how many of them hold x,
 *   computed on the host in float64 and handed over as doubles in a table (below); an n-gram the table does not hold has
 *   default_idf (= log(D)).  The device takes no logarithm.  Without a table every idf is exactly 1 (n-gram TF cosine consensus).
 *  Score.  With v(x) = tf(x) * idf(x), hypothesis h, reference r and order n:
 *   val_n(h, r) = sum over the distinct x of h, in order of first position, of min(v_h(x), v_r(x)) * v_r(x);
 *   with |v|_n = sqrt(sum over the order's distinct x, in order of first position, of v(x)^2): if |v_h|_n * |v_r|_n != 0 the
 *   value is divided by that product, else it stays as it is (0); then it is multiplied by exp(-(L_h - L_r)^2 / (2 sigma^2))
 *   (sigma = inf: exactly 1).
 *   c_n(h) = (sum_j w_j * val_n(h, r_j)) / (sum_j w_j) over the PRESENT references j of the row's dialog in index order, w_j >= 0
 *   (NULL weights: every w_j = 1, CIDEr-D's 1 / m).  A present reference with L = 0 adds 0 and still counts in the denominator.
 *   reward = 10 * (c_1 + c_2 + c_3 + c_4) / 4.
 *   The reward and every c_n are 0 for an absent hypothesis, a hypothesis with L = 0, a dialog without a present reference, a
 *   weight sum of 0, and a hyp_group outside [0, G).
 *  Limits.  L <= 64 for hypotheses and references (a hypothesis then has at most 64 + 63 + 62 + 61 = 250 n-grams, fewer than the
 *   256 lanes of a workgroup); at most 128 references per dialog.
 *
 * THE TABLE is open addressing with exact keys: keys int32 [cap, 4], the n-gram's tokens padded with -1 (so the order is part of
 * the key and no hash collision can alias two n-grams); values double [cap]; cap a power of two; an empty slot has
 * UNIMM_NGRAM_EMPTY in its first key word.  The home slot of a key (k0, k1, k2, k3) is h & (cap - 1), with, in uint32 arithmetic,
 *   h = UNIMM_NGRAM_HASH_BASIS;  for i = 0 .. 3: h = (h ^ (uint32) k_i) * UNIMM_NGRAM_HASH_PRIME;  h = h ^ (h >> 16)
 * (FNV-1a over the four words, then one fold); probing is linear, slot + 1 wrapping at cap, and ends at the key, at an empty slot
 * (-> default_idf) or after cap probes (-> default_idf).  unimm_amd/reward.py restates the hash in numpy and builds the table.
 *
 * THE KERNEL.  One 256-thread workgroup per hypothesis row; wave w holds order n = w + 1 and lane p the window at position p.
 * All arithmetic is fp64; every sum is a serial chain in index order (n-gram position, then reference index), there are no atomics
 * and no arrival counters, so equal inputs give equal bits on every launch and a row's result depends on that row's inputs
 * alone -- not on S, the row's position or the grid.  `reward` is the one rounding of the fp64 value to fp32.  A reference of
 * weight exactly 0 adds exactly 0 to both sums and is not walked.
 *
 * LENGTHS live on the device and a call never synchronises, so the limits on them are held through two bounds the caller
 * vouches for: max_hyp_len / max_ref_len, the largest length (counting the [SEP]) of any row.  UNIMM_E_SHAPE when a bound is
 * below 0, above 65 (L > 64) or above its row stride; a device length above its bound is read as the bound, so no row is ever
 * read past its stride whatever the device holds (unimm_amd/reward.py refuses such input on the host).
 * args NULL: UNIMM_E_ARG; S < 0: UNIMM_E_SHAPE; S = 0 returns UNIMM_OK without a launch and without looking further (the
 * address of an empty array may be NULL).  Otherwise, before any launch, UNIMM_E_ARG: a mandatory pointer NULL (hyp, hyp_len,
 * hyp_group, ref, ref_len, reward), one of table_keys / table_idf without the other, sigma <= 0 or NaN.  UNIMM_E_SHAPE: G < 1,
 * M < 1 or M > UNIMM_REWARD_MAX_REFS, a stride below 1, the bounds above, and with a table a cap that is no power of two.  A
 * refused call writes nothing.  `stream` is a hipStream_t passed as void*, pointers are device pointers and the call only enqueues work
 * (no allocation, no synchronisation): the conventions of unimm_hip.h, whose UNIMM_* result codes it returns. */
#ifndef UNIMM_REWARD_H
#define UNIMM_REWARD_H

#include "unimm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int unimm_reward_version(void);   /* ABI version of this library, bumped on any signature change */

#define UNIMM_REWARD_MAX_LEN 64
#define UNIMM_REWARD_MAX_REFS 128
#define UNIMM_REWARD_ORDERS 4
#define UNIMM_NGRAM_EMPTY (-2)
#define UNIMM_NGRAM_HASH_BASIS 2166136261
#define UNIMM_NGRAM_HASH_PRIME 16777619
typedef struct {
  const int32_t* hyp; const int32_t* hyp_len; const int32_t* hyp_group;   /* int32 [S, ldh], [S], [S]: group = the row's dialog */
  const int32_t* ref; const int32_t* ref_len;                             /* int32 [G, M, ldr], [G, M] */
  const float* ref_weight;                                                /* fp32 [G, M], or NULL = uniform */
  const int32_t* table_keys; const double* table_idf;                     /* int32 [cap, 4], double [cap]; both NULL = every idf 1 */
  float* reward;                                                          /* fp32 [S] */
  double* per_order;                                                      /* double [S, 4] = the c_n, or NULL */
  double default_idf, sigma;
  int32_t S, ldh, G, M, ldr, cap, max_hyp_len, max_ref_len;
} unimm_ngram_reward_args;
int unimm_ngram_reward(const unimm_ngram_reward_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIMM_REWARD_H */
