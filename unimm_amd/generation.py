"""Answer generation: beam search over the generative (prefix-LM) mask with a per-layer key/value cache.

Why a cache is exact.  Under the generative mask (utils/data_utils.py:199-210; `oracle/masks.py` restates it), with context
length c (dialog `[CLS] caption [SEP] q1 [SEP] a1 ... q_r [SEP]` in positions [0, c)):

    context rows [1, c)   attend [1, c)                       -- never column 0, never the answer
    answer row c + k      attends [1, c + k]                  -- causal
    copy row of token k   attends [1, c + k) + itself         -- a [MASK] with answer token k's position id; predicts token k
    regions               attend text [1, c)                  (co-attention mask)
    column 0 (CLS)        is attended by nobody but CLS itself

so the image stream and the context rows never depend on the answer, answer row k depends on earlier answer rows only and
the copy row of token k on the context and answer rows < k.  A dialog is PREFILLED once (context + image through the whole
encoder: the shared-context pass of `scoring.py`, which keeps every text layer's context K / V and every connection layer's
region K1 / V1), and decode step k pushes exactly two new text rows per hypothesis through the blocks: answer row k-1 (its
K / V joins the hypothesis's private cache afterwards) and copy row k (its logits choose token k).  Step 0 needs no decode:
the prefill runs the one-token sequence `context [SEP] [MASK]`, whose copy row IS copy row 0.  Consequently the log p of a
generated answer equals `sequence_log_likelihood` of the completed sequence.

Answer token k of dialog g has position id position_ids[g, c-1] + 1 + k and segment token_type_ids[g, c-1] ^ 1
(`oracle/masks.py::_layout`: the segment toggles for the answer); the copy rows are [MASK] (103) with the same ids.

Search semantics (k = tokens generated so far, excluding [SEP]):

* Step k: for each live hypothesis, log-softmax over the vocabulary of its copy row's logits; then -inf for the ids in
  `banned_tokens`, for [SEP] (102) while k < min_answer_len, and for every id other than [SEP] once k reaches the dialog's
  limit min(max_answer_len, (T - c) // 2 - 1) (so that the completed sequence fits in T untruncated), which forces the end.
  No renormalisation after banning: scores stay comparable with `sequence_log_likelihood`.
* Candidates: each live hypothesis proposes its top `beams` tokens (value desc, id asc); a candidate's score is the parent's
  cumulative log p plus the token's log p (fp32).  Candidates are ordered by (score desc, parent slot asc, token id asc);
  candidates of score -inf are never taken.
* The walk over the ordered candidates: a [SEP] candidate becomes a finished hypothesis (final score
  logp / (k + 1) ** length_penalty) while the dialog has fewer than `beams` finished ones; any other candidate takes a live
  slot; the walk ends when `beams` live slots are filled.
* A dialog stops when it has `beams` finished hypotheses or no live hypothesis left.
* Output: the `beams` best finished hypotheses by (final score desc, finishing step asc, walk order); a dialog that finished
  fewer pads with zero tokens, length 0 and score / logp -inf.
* beams = 1 is greedy decoding; length_penalty = 0 returns the summed log p of val_lm.py, 1 the token mean of val_avg_lm.py.

`beam_search` is written against an abstract step function (tests drive it with a table model on the CPU); `generate_answers`
supplies the engine's: the prefill, the caches and the decode step are a `decoding.DecodeSide` (the existing NT GEMM / LayerNorm
kernels on M = 2 * slots rows with the engine's `_post_attn` after each attention, `unimm_attn_decode` for text self-attention,
`unimm_attn_fwd` against the cached regions for the text half of a connection layer, the MLM head on the copy rows), followed by
`unimm_lm_topk` on the fp32 logits, with `unimm_kv_cache_update` (append + reorder of the private caches of all text layers)
between steps.  Beam selection runs as
torch ops on the [G, beams * beams] candidates; the only device->host synchronisation of a step is the "all dialogs
stopped" flag.  Inference only, bf16 engine with the connection layers.

Sampling (`samples` > 0, `sample_search`): `samples` independent hypothesis slots per dialog, each DRAWING token k from its copy
row's distribution after the same step rules (banned ids, [SEP] banned below min_answer_len and forced at the dialog's limit),
then top-k, temperature and nucleus filtering -- `unimm_lm_sample`, whose header comment fixes the order.  The model part of the
step is the beam search's; a slot never changes parent, so its private caches only grow: the new K | V row of every text layer is
appended in place.  A slot is finished when it draws [SEP]; the loop ends when every slot is (one synchronisation per step) or
after max_answer_len + 1 steps.  Draw j of dialog g at step k uses key = dropout.make_key(seed, k, SAMPLE_SITE) and stream
sample_streams[g] * samples + j, and depends on nothing else but the row's logits: a caller that passes its own dialog ids as
`sample_streams` gets the same draws for a dialog wherever it stands in the batch (up to the batch dependence of the logits
themselves).  Every token comes with log p under the unmodified distribution (step_logp, summed in logp: equal to
`sequence_log_likelihood` of the completed sequence, as for beams) and log q under the one sampled from (step_logq).  Samples are
returned in draw order, not sorted.

Per-draw decoding parameters and the greedy slot (one rollout for self-critical training).  `temperature`, `top_k` and `top_p` each
take a scalar or a sequence of `samples` values, value j for draw j of every dialog.  `greedy=True` adds one more slot per dialog
to the SAME prefill and decode steps: dialog g then owns slots g * (N + 1) + j, j < N the samples and j = N a slot that decodes
greedily (top_k = 1, temperature 1, top_p 1: its one kept id is the first of the rank order, the token beams = 1 takes, with
log q = 0).  The samples keep their streams sample_streams[g] * N + j, keys and step rules, so they are the draws of the call
without the greedy slot (up to the batch dependence of the logits); the greedy answer comes back in `GeneratedAnswers.greedy`,
shaped like a beams = 1 result.  With per-draw parameters or a greedy slot the draw is `unimm_lm_sample_rows` (the same kernel
with per-row parameters, ABI 24); a call that uses neither launches `unimm_lm_sample` as before.  The loop ends when every slot,
the greedy one included, has finished.

Rules that depend on what a hypothesis has said (`no_repeat_ngram_size`, `repetition_penalty`, `repeat_scope`).  At step k a slot's
history sources are its own answer tokens a[0, k) ([SEP] is never among them) and, with repeat_scope="dialog", the dialog's context
tokens input_ids[g, 1:c) as a second source ([CLS] excluded).  no_repeat_ngram_size = n (0 = off, at most 8): once k >= n - 1, id t
is banned for the slot when some window s[e-n+1 .. e] of ONE source has s[e-n+1 .. e) == a[k-n+1 .. k) and s[e] == t -- overlapping
windows count, no window spans the context/answer boundary, n = 1 bans every id of the sources, and [SEP] is never banned by the
rule (the forced end always keeps one eligible id).  Such a ban is an entry of `banned_tokens` for that slot and step: -inf after
the log-sum-exp, no renormalisation, so step_logp is still `sequence_log_likelihood` of the completed answer.  It works with any
`beams` and `samples` and applies to the greedy slot too.  repetition_penalty = r (1 = off, finite, > 0) shapes SELECTION only:
every id i of the sources is ranked, filtered and drawn by x'_i = x_i > 0 ? x_i * fp32(1 / r) : x_i * r, every other id by x_i;
step_logq is the log-probability under that distribution (what `PolicyObjective(mode="ratio")` weighs by), step_logp stays
x_i - logsumexp(x).  A beam's cumulative score is the model's log p, and a penalised ranking across hypotheses would be a different
search, so the penalty is admitted for beams = 1 (which takes the first id of the rank order on x' and reports its raw log p, as
the greedy slot of a sampling call does) and for sampling.  With any of the rules on, every step -- step 0 on the prefill's row
included -- launches `unimm_lm_topk_hist` / `unimm_lm_sample_hist` (the two kernels with a per-row history: a device int32
[slots, width] table that `track_history` reorders by parent and appends to, and the context table built once per call); with all
of them off the call launches exactly the kernels named above.

Speculative greedy decoding (`draft`, `draft_len`; unimm_amd/speculative.py states the rounds).  The mask argument at the top covers
more than one step at a time: answer row k depends on earlier answer rows only and copy row k on the context and the answer rows
before k, so the draft_len + 1 pairs (answer row n-1+j, copy row n+j) of consecutive steps go through the blocks in ONE pass, as
long as every new row attends the answer rows of the pairs up to its own, itself if it is a copy row, and no other new row
(`unimm_attn_verify`).  A draft model -- either class, its own depth and widths, the model's vocabulary and inputs -- proposes
draft_len greedy tokens per round; the model verifies them in that one pass, keeps the longest prefix it would have produced
itself plus one token of its own (each with ITS log p), appends the kept rows to its cache in place (`unimm_kv_cache_append`) and
the draft's cache rolls back.  The result is the beams = 1 result (tokens, lengths, step_logp, logp, scores; up to the batch
dependence of the logits) with `.speculation` = rounds, drafted and accepted tokens per dialog.  beams = 1 only, no
history rules; with draft=None nothing here runs and a call launches what it always launched.

Speculative SAMPLING (`samples=N, draft=..., draft_accept="rejection"`; "match", the default, is the greedy form above and still
refuses `samples`).  The draft DRAWS its proposals from its own filtered distribution Q~; the model's one pass is followed by one
`unimm_lm_spec_verify` launch that accepts each draft with probability min(1, P~ / Q~) or draws from the normalised residual
max(0, P~ - Q~), P~ the distribution the plain sampling call draws from -- so the answers are distributed exactly as that call's,
only in fewer passes of the model.  The result is sampling-shaped: the samples in draw order with step_logp (the model's log p) and
step_logq (log P~ of the emitted token), `.greedy` when asked (a top_k = 1 slot on both sides), `.speculation` with [G, N]
counters.  Keys are per ABSOLUTE step and the streams those of the plain call; a seed fixes the answers for a GIVEN draft_len only
(whether a step is a drafted row or the bonus row, a plain draw, depends on draft_len): the distribution is the same, the draws not.
Needs samples >= 1 and a draft; every refusal of the greedy form applies (the history rules included), and `beams` follows the
sampling call's rule.

Ensemble and contrastive decoding (`ensemble=[partners]`, `ensemble_weights`, `ensemble_mode`, `plausibility`).  The call's model
is member 0 and `ensemble` names 1 to 4 partners of either class -- their own depth, widths and layer schedule, the model's
vocabulary and inputs, each on a bf16 engine of its own (`policy.frozen_reference(model)` for a second copy of the same weights).
Every member gets a `DecodeSide` with the same slots and groups; a step pushes the SAME tokens through every side, one
`unimm_lm_mix` launch (the extension library libunimm_mix.so, bound by unimm_amd/mix.py) turns the K logits blocks into one
[slots, Vpad] block (at step 0: the K prefill rows), and the selection launch of the plain call -- top-k, a draw, with or without a history -- reads that block.  `reorder` / `append_in_place` are applied
to every side; the searches see a step function and do not change.  ensemble_mode="prob" (the default) is the arithmetic mixture
z_i = log sum_m w_m p_m(i), the usual checkpoint ensemble: weights >= 0 that sum to 1 (within 1e-6), w_0 > 0, default uniform;
the mixed row sums to 1, so step_logp = log sum_m w_m p_m(token).  "logit" is the log-linear mixture z_i = sum_m w_m x_m,i with
finite weights of any sign, w_0 > 0; softmax(z) is the normalised product of the p_m ** w_m and step_logp the log-probability
under it.  plausibility = alpha in (0, 1) cuts, before the selection, every id but [SEP] whose logit under THE MODEL (member 0) is
below its best eligible logit + fp32(log alpha) -- p_0(i) < alpha max p_0 -- so that weights (1 + b, -b) with a cut are contrastive
decoding (expert minus amateur on the ids the expert finds plausible); step_logp is then normalised over the plausible set.  The
step rules, beams, sampling with per-draw parameters, greedy=True and length_penalty work as in the plain call, the history rules
too but not together with a cut (a ban could empty the plausible set).  Refused on the host before anything is staged: `ensemble`
with `draft`, no or more than 4 partners, a partner that is the model, a repeated partner or a shared engine, a partner of another
device, engine, vocabulary, input shape or head size, weights of the wrong number or outside the mode's rule, an unknown mode,
`plausibility` outside [0, 1), and `ensemble_weights` or a cut without `ensemble`.  With ensemble=None nothing here runs and a call
launches what it always launched.  A step costs K decode steps plus the mix (tools/bench_generate.py --ensemble K).
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass

import numpy as np
import torch

from . import dropout as DR
from . import lib as L
from .decoding import F32, SEP, DecodeSide, answer_ids  # noqa: F401  (answer_ids: stated there for the side, part of this module)

MAX_BEAMS = 16
MAX_SAMPLES = 16                               # unimm_attn_decode takes 2 * slots <= 32 query rows per dialog
SEP_BANNED, SEP_FORCED = 1, 2                  # per-row flags of unimm_lm_topk / unimm_lm_sample
SAMPLE_SITE = zlib.crc32(b"generate.sample") & 0xFFFFFFFF   # the engine's dropout sites are crc32 of their parameter names


@dataclass
class Speculation:
    """What a speculative call (`draft=`) did, per dialog."""
    rounds: int               # draft + verify rounds of the call
    drafted: torch.Tensor     # int64 [G]: tokens the draft proposed while the dialog was live (draft_len per round)
    accepted: torch.Tensor    # int64 [G]: ... of which the model kept
    per_round: torch.Tensor | None = None   # int64 [rounds, G]: accepted drafts of each round, -1 where the dialog had finished


@dataclass
class GeneratedAnswers:
    tokens: torch.Tensor    # int64 [G, beams, max_answer_len + 1]: answer tokens then [SEP], zero-padded
    lengths: torch.Tensor   # int64 [G, beams], including the [SEP]
    scores: torch.Tensor    # fp32 [G, beams]: logp / lengths ** length_penalty
    logp: torch.Tensor      # fp32 [G, beams]: summed log p
    step_logp: torch.Tensor  # fp32 [G, beams, max_answer_len + 1]: the log p of each token (an extension: per-step checks)
    step_logq: torch.Tensor | None = None   # sampling only: the log q of each token under the distribution it was drawn from
    greedy: "GeneratedAnswers | None" = None   # samples with greedy=True: the greedy answers, shaped like a beams = 1 result
    speculation: Speculation | None = None  # draft= only (unimm_amd/speculative.py)


def answer_limits(context_len, T, max_answer_len):
    """Tokens dialog g may generate before its [SEP]: min(max_answer_len, (T - c) // 2 - 1)."""
    c = np.asarray(context_len, dtype=np.int64).reshape(-1)
    return np.minimum(max_answer_len, (T - c) // 2 - 1)


def check_model(m, draft=False):
    """What a decode side needs of its model -- the call's, or (draft) its draft: the bf16 engine, the connection layers and text
    heads of 64 (NotImplementedError / ValueError, in the words of each)."""
    dtype, D = getattr(m, "compute_dtype", "bf16"), m.config.hidden_size // m.config.num_attention_heads
    if dtype != "bf16":
        raise (ValueError(f"generate_answers: draft must run on the bf16 engine (compute_dtype='bf16'), got {dtype!r}") if draft
               else NotImplementedError("generate_answers runs on the bf16 engine"))
    if not m.config.with_coattention:
        raise (ValueError("generate_answers: draft needs the connection layers (with_coattention)") if draft
               else NotImplementedError("generate_answers needs the connection layers (with_coattention)"))
    if D != 64:
        whose = "draft's " if draft else ""
        raise ValueError(f"generate_answers: {whose}text head size {D} (unimm_attn_decode takes 64)")


def check_request(context_len, T, beams, max_answer_len, min_answer_len):
    """The refused cases (ValueError): -> per-dialog limits (np.int64 [G])."""
    if not 1 <= int(beams) <= MAX_BEAMS:
        raise ValueError(f"generate_answers: beams must be in [1, {MAX_BEAMS}], got {beams}")
    if max_answer_len < 0 or min_answer_len < 0 or min_answer_len > max_answer_len:
        raise ValueError(f"generate_answers: need 0 <= min_answer_len <= max_answer_len (got {min_answer_len}, {max_answer_len})")
    c = np.asarray(context_len, dtype=np.int64).reshape(-1)
    if (c < 2).any() or (c > T).any():
        raise ValueError("generate_answers: every context must hold [CLS] and at least one token (2 <= context_len <= T)")
    lim = answer_limits(c, T, max_answer_len)
    bad = np.nonzero(lim < min_answer_len)[0]
    if bad.size:
        g = int(bad[0])
        raise ValueError(f"generate_answers: dialog {g} (context {int(c[g])} of T = {T}) has room for {max(int(lim[g]), 0)} answer "
                         f"tokens, fewer than min_answer_len = {min_answer_len}")
    return lim


def row_flags(k, limits, min_answer_len):
    """int32 flags (any shape) of rows that stand at step k (an int, or int64 of limits' shape or broadcastable to it): SEP_BANNED
    while k < min_answer_len, SEP_FORCED once k reaches the dialog's limit."""
    return (torch.where(limits <= k, SEP_FORCED, 0) | (k < min_answer_len) * SEP_BANNED).to(torch.int32)


def step_flags(k, limits, beams, min_answer_len):
    """int32 [G * beams] flags of step k: row_flags of the dialogs, per hypothesis slot."""
    return row_flags(k, limits, min_answer_len).repeat_interleave(beams)


def beam_search(step, G, beams, limits, max_answer_len, min_answer_len=1, length_penalty=0.0, device="cpu"):
    """Run the search of the module docstring.  step(k, parent, token, flags) -> (vals fp32 [G*beams, beams], ids [G*beams, beams]):
    the top-`beams` log p (value desc, id asc; banned ids -inf) of every hypothesis slot at step k, where slot s continues slot
    parent[s] of the previous step with answer token k-1 = token[s] (k = 0: one root per dialog, slot g * beams; the other
    slots' rows are ignored).  limits: per-dialog token limits (answer_limits)."""
    S, W, NEG = G * beams, max_answer_len + 1, float("-inf")
    dev = torch.device(device)
    limits = torch.as_tensor(np.asarray(limits), dtype=torch.int64).to(dev)
    cum = torch.full((G, beams), NEG, dtype=F32, device=dev)
    cum[:, 0] = 0.0
    hist = torch.zeros((S, W), dtype=torch.int64, device=dev)
    hist_lp = torch.zeros((S, W), dtype=F32, device=dev)
    parent = torch.arange(S, device=dev)
    token = torch.zeros(S, dtype=torch.int64, device=dev)
    alive = torch.ones(G, dtype=torch.bool, device=dev)
    # finished hypotheses, in finishing order; entry `beams` of each dialog is a sink for the candidates not accepted
    fin_tok = torch.zeros((G, beams + 1, W), dtype=torch.int64, device=dev)
    fin_lp = torch.zeros((G, beams + 1, W), dtype=F32, device=dev)
    fin_len = torch.zeros((G, beams + 1), dtype=torch.int64, device=dev)
    fin_logp = torch.full((G, beams + 1), NEG, dtype=F32, device=dev)
    fin_score = torch.full((G, beams + 1), NEG, dtype=F32, device=dev)
    nfin = torch.zeros(G, dtype=torch.int64, device=dev)
    gbase = (torch.arange(G, device=dev) * beams)[:, None]
    for k in range(max_answer_len + 1):
        vals, ids = step(k, parent, token, step_flags(k, limits, beams, min_answer_len).to(dev))
        vals = vals.to(dev, F32).view(G, beams, beams)
        ids = ids.to(dev, torch.int64).view(G, beams, beams)
        score = (cum[:, :, None] + vals).masked_fill(~alive[:, None, None], NEG).view(G, beams * beams)
        order = torch.sort(score, dim=1, descending=True, stable=True).indices   # (score desc, parent asc, rank = id asc)
        sc = score.gather(1, order)
        tk = ids.view(G, beams * beams).gather(1, order)
        tv = vals.reshape(G, beams * beams).gather(1, order)
        par = order // beams                                                  # parent slot inside the dialog
        finite = sc > NEG
        is_sep = finite & (tk == SEP)
        is_live = finite & (tk != SEP)
        nlive = torch.cumsum(is_live.to(torch.int64), 1)
        reached = (nlive - is_live.to(torch.int64)) < beams                   # the walk ends at the beams-th live candidate
        take = is_live & (nlive <= beams)
        cand_fin = is_sep & reached
        frank = nfin[:, None] + torch.cumsum(cand_fin.to(torch.int64), 1) - 1
        accept = cand_fin & (frank < beams)
        # finished: the parent's history + [SEP] at position k
        ftok = hist.view(G, beams, W).gather(1, par[:, :, None].expand(-1, -1, W)).clone()
        ftok[:, :, k] = SEP
        flp = hist_lp.view(G, beams, W).gather(1, par[:, :, None].expand(-1, -1, W)).clone()
        flp[:, :, k] = tv
        fidx = torch.where(accept, frank, beams)
        fin_tok.scatter_(1, fidx[:, :, None].expand(-1, -1, W), ftok)
        fin_lp.scatter_(1, fidx[:, :, None].expand(-1, -1, W), flp)
        fin_len.scatter_(1, fidx, torch.full_like(fidx, k + 1))
        fin_logp.scatter_(1, fidx, sc)
        fin_score.scatter_(1, fidx, sc / float((k + 1) ** length_penalty))
        nfin = nfin + accept.sum(1)
        # live: slot rank = order among the taken candidates
        lidx = torch.where(take, nlive - 1, beams)
        new_par = torch.cat([gbase.expand(G, beams) + torch.arange(beams, device=dev), gbase], 1)
        new_par = new_par.scatter(1, lidx, gbase + par)[:, :beams]
        new_tok = torch.zeros((G, beams + 1), dtype=torch.int64, device=dev).scatter(1, lidx, tk)[:, :beams]
        new_cum = torch.full((G, beams + 1), NEG, dtype=F32, device=dev).scatter(1, lidx, sc)[:, :beams]
        new_lp = torch.zeros((G, beams + 1), dtype=F32, device=dev).scatter(1, lidx, tv)[:, :beams]
        parent, token = new_par.reshape(S), new_tok.reshape(S)
        hist, hist_lp = hist[parent], hist_lp[parent]
        hist[:, k] = token
        hist_lp[:, k] = new_lp.reshape(S)
        cum = new_cum
        alive = alive & (nfin < beams) & take.any(1)
        if not bool(alive.any()):                                             # the step's one device -> host synchronisation
            break
    fs = fin_score[:, :beams]
    order = torch.sort(fs, dim=1, descending=True, stable=True).indices
    return GeneratedAnswers(tokens=fin_tok[:, :beams].gather(1, order[:, :, None].expand(-1, -1, W)),
                            lengths=fin_len[:, :beams].gather(1, order), scores=fs.gather(1, order),
                            logp=fin_logp[:, :beams].gather(1, order),
                            step_logp=fin_lp[:, :beams].gather(1, order[:, :, None].expand(-1, -1, W)))


def _per_draw(value, samples, name):
    """A scalar, or a sequence of `samples` values (value j for draw j) -> (list of `samples` values, was it a sequence)."""
    if torch.is_tensor(value):
        value = value.tolist()
    if isinstance(value, (list, tuple, np.ndarray)):
        vals = [v.item() if isinstance(v, np.generic) else v for v in value]
        if len(vals) != int(samples):
            raise ValueError(f"generate_answers: {len(vals)} {name} values for {samples} samples (a scalar, or one value per draw)")
        return vals, True
    return [value] * int(samples), False


def check_sampling(samples, beams, temperature, top_k, top_p, greedy=False):
    """The refused sampling requests (ValueError) -> (temperature fp32 [N], top_k int32 [N], top_p fp32 [N], per_draw): the
    decoding parameters of draw j, and whether any of the three was given per draw."""
    if not 1 <= int(samples) <= MAX_SAMPLES:
        raise ValueError(f"generate_answers: samples must be in [0, {MAX_SAMPLES}], got {samples}")
    if int(beams) != 1:
        raise ValueError(f"generate_answers: samples > 0 draws independent answers and needs beams = 1, got beams = {beams}")
    if greedy and int(samples) + 1 > MAX_SAMPLES:
        raise ValueError(f"generate_answers: greedy=True adds a slot per dialog, and samples + 1 = {int(samples) + 1} slots exceed "
                         f"{MAX_SAMPLES}: unimm_attn_decode takes 2 * slots <= 32 query rows per dialog")
    (ts, st), (ks, sk), (ps, sp) = (_per_draw(v, samples, n) for v, n in ((temperature, "temperature"), (top_k, "top_k"),
                                                                          (top_p, "top_p")))
    for t, k, p in zip(ts, ks, ps):
        if not (t > 0 and math.isfinite(t)):
            raise ValueError(f"generate_answers: temperature must be positive and finite, got {t}")
        if int(k) != k or k < 0:
            raise ValueError(f"generate_answers: top_k must be an integer >= 0 (0 = off), got {k}")
        if not 0.0 < p <= 1.0:
            raise ValueError(f"generate_answers: top_p must be in (0, 1] (1 = off), got {p}")
    return (np.asarray(ts, dtype=np.float32), np.asarray([int(k) for k in ks], dtype=np.int32), np.asarray(ps, dtype=np.float32),
            st or sk or sp)


def slot_parameters(G, temperature, top_k, top_p, greedy=False):
    """Per-draw parameters (check_sampling) -> the same per hypothesis slot, (fp32, int32, fp32) [G * slots]: dialog g owns slots
    g * slots + j, the draws in order and then, with `greedy`, the greedy slot (temperature 1, top_k 1, top_p 1)."""
    extra = ((1.0,), (1,), (1.0,)) if greedy else ((), (), ())
    return tuple(np.tile(np.concatenate([a, np.asarray(e, dtype=a.dtype)]), G) for a, e in zip((temperature, top_k, top_p), extra))


MAX_NGRAM, MAX_HISTORY, MAX_CONTEXT = 8, 128, 256  # unimm_lm_history: ngram, ldh and ldc bounds
REPEAT_SCOPES = ("answer", "dialog")


def check_constraints(no_repeat_ngram_size=0, repetition_penalty=1.0, repeat_scope="answer", beams=1):
    """The refused history rules (ValueError) -> None when both are off, else dict(ngram, penalty, scope)."""
    n, r = no_repeat_ngram_size, repetition_penalty
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n <= MAX_NGRAM:
        raise ValueError(f"generate_answers: no_repeat_ngram_size must be an integer in [0, {MAX_NGRAM}] (0 = off), got {n!r}")
    if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)) or not (math.isfinite(r) and r > 0):
        raise ValueError(f"generate_answers: repetition_penalty must be finite and > 0 (1 = off), got {r!r}")
    if repeat_scope not in REPEAT_SCOPES:
        raise ValueError(f"generate_answers: repeat_scope must be one of {REPEAT_SCOPES}, got {repeat_scope!r}")
    if float(np.float32(r)) != 1.0 and int(beams) > 1:
        raise ValueError(f"generate_answers: repetition_penalty = {r} needs beams = 1 (got beams = {beams}): a beam's cumulative score is "
                         f"the model's log p, and ranking hypotheses by penalised logits would be a different search")
    if n == 0 and float(np.float32(r)) == 1.0:
        return None
    return dict(ngram=int(n), penalty=float(np.float32(r)), scope=repeat_scope)


MAX_PARTNERS = 4                               # unimm_lm_mix takes K <= 5 rows: the model and four partners
ENSEMBLE_MODES = ("prob", "logit")
_PARTNER_CONFIG_KEYS = ("vocab_size", "v_feature_size", "type_vocab_size", "max_position_embeddings")


def check_partner(model, partner, index):
    """What member `index` >= 1 of an ensemble must be (ValueError) -> its pre-training model: a model of either class, not the
    call's model, on its device and the bf16 engine, with the connection layers, text heads of 64, the model's vocabulary and
    inputs.  Depth, widths and the layer schedule are its own."""
    from .policy import _pretraining_model
    p, who = _pretraining_model(partner), f"ensemble member {index}"
    if not (hasattr(p, "config") and hasattr(p, "_engine") and hasattr(p, "compute_dtype")):
        raise ValueError(f"generate_answers: {who} must be a BertForMultiModalPreTraining or a VisualDialogEncoder, got "
                         f"{type(partner).__name__}")
    if p is model or p._engine is model._engine:
        raise ValueError(f"generate_answers: {who} is the model itself (or shares its engine): every member keeps its own key/value "
                         "caches; pass a separate model, or policy.frozen_reference(model) for a second copy of the same weights")
    if p.compute_dtype != "bf16":
        raise ValueError(f"generate_answers: {who} must run on the bf16 engine (compute_dtype='bf16'), got {p.compute_dtype!r}")
    if not p.config.with_coattention:
        raise ValueError(f"generate_answers: {who} needs the connection layers (with_coattention)")
    D = p.config.hidden_size // p.config.num_attention_heads
    if D != 64:
        raise ValueError(f"generate_answers: {who} has text head size {D} (unimm_attn_decode takes 64)")
    diff = [k for k in _PARTNER_CONFIG_KEYS if getattr(p.config, k, None) != getattr(model.config, k, None)]
    if diff:
        raise ValueError(f"generate_answers: {who} must read the model's inputs and predict over its vocabulary; its config differs "
                         f"in {', '.join(diff)}")
    if p._device() != model._device():
        raise ValueError(f"generate_answers: {who} is on {p._device()}, the model on {model._device()}: move it with .to()")
    return p


def check_ensemble(model, ensemble, ensemble_weights=None, ensemble_mode="prob", plausibility=0.0, draft=None,
                   no_repeat_ngram_size=0, repetition_penalty=1.0):
    """The refused ensemble requests (ValueError, before anything is staged) -> None without `ensemble`, else dict(partners: the
    partners' pre-training models, weights: K floats with the model's first, mode, log_alpha: fp32(log plausibility), -inf = off)."""
    a = plausibility
    if isinstance(a, bool) or not isinstance(a, (int, float, np.integer, np.floating)) or not 0.0 <= a < 1.0:
        raise ValueError(f"generate_answers: plausibility must be in [0, 1) (0 = off), got {a!r}")
    if ensemble_mode not in ENSEMBLE_MODES:
        raise ValueError(f"generate_answers: ensemble_mode must be one of {ENSEMBLE_MODES}, got {ensemble_mode!r}")
    if ensemble is None:
        if ensemble_weights is not None or a > 0:
            raise ValueError("generate_answers: ensemble_weights and plausibility shape the mixture of an ensemble and need partner "
                             "models (ensemble=[...])")
        return None
    if draft is not None:
        raise ValueError("generate_answers: ensemble with draft: a speculative call verifies ONE model's tokens; drop one of the two")
    if isinstance(ensemble, torch.nn.Module) or not isinstance(ensemble, (list, tuple)):
        raise ValueError(f"generate_answers: ensemble must be a sequence of 1 to {MAX_PARTNERS} partner models, got "
                         f"{type(ensemble).__name__}")
    if not 1 <= len(ensemble) <= MAX_PARTNERS:
        raise ValueError(f"generate_answers: ensemble takes 1 to {MAX_PARTNERS} partner models (unimm_lm_mix mixes at most "
                         f"{MAX_PARTNERS + 1} rows), got {len(ensemble)}")
    partners = []
    for i, m in enumerate(ensemble):
        p = check_partner(model, m, i + 1)
        if any(p is q or p._engine is q._engine for q in partners):
            raise ValueError(f"generate_answers: ensemble member {i + 1} is an earlier member again (or shares its engine): every "
                             "member keeps its own key/value caches; use policy.frozen_reference for a copy")
        partners.append(p)
    K = len(partners) + 1
    if ensemble_weights is None:
        w = [1.0 / K] * K
    else:
        w = ensemble_weights.tolist() if torch.is_tensor(ensemble_weights) or isinstance(ensemble_weights, np.ndarray) \
            else list(ensemble_weights)
        if len(w) != K:
            raise ValueError(f"generate_answers: {len(w)} ensemble_weights for {K} members (the model's first, then one per partner)")
        if any(isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) for v in w):
            raise ValueError(f"generate_answers: ensemble_weights must be finite numbers, got {w!r}")
        w = [float(v) for v in w]
    if not w[0] > 0:
        raise ValueError(f"generate_answers: the model's own weight (ensemble_weights[0]) must be > 0, got {w[0]}")
    if ensemble_mode == "prob" and (min(w) < 0 or abs(sum(w) - 1.0) > 1e-6):
        raise ValueError(f"generate_answers: ensemble_mode='prob' mixes probabilities: the weights must be >= 0 and sum to 1 "
                         f"(within 1e-6), got {w!r}")
    if a > 0 and (no_repeat_ngram_size or float(np.float32(repetition_penalty)) != 1.0):
        raise ValueError("generate_answers: plausibility > 0 with no_repeat_ngram_size or repetition_penalty: a ban of the history "
                         "rules could empty the plausible set; drop the cut, or the rules")
    log_alpha = float(np.float32(np.log(np.float64(a)))) if a > 0 else float("-inf")
    return dict(partners=partners, weights=w, mode=ensemble_mode, log_alpha=log_alpha)


def new_history(S, width, device="cpu"):
    """The answer history of S hypothesis slots: dict(hist int32 [S, width], len int32 [S]), empty."""
    dev = torch.device(device)
    return dict(hist=torch.zeros((S, max(int(width), 1)), dtype=torch.int32, device=dev),
                len=torch.zeros(S, dtype=torch.int32, device=dev))


def track_history(h, k, token, parent=None):
    """Bring the history `h` (new_history) to step k from the arguments a step function gets: slot s continues slot parent[s]
    (beam search; None: itself, sampling) with answer token k-1 = token[s].  Afterwards h["hist"][s, :h["len"][s]] are the answer
    tokens a[0, k) of slot s.  Step 0 starts every slot empty."""
    if k == 0:
        h["len"].zero_()
        return h
    if parent is not None:
        h["hist"] = h["hist"][parent.to(h["hist"].device, torch.int64)]
    if k - 1 < h["hist"].shape[1]:
        h["hist"][:, k - 1] = token.to(h["hist"].device, torch.int32)
    h["len"].fill_(min(k, h["hist"].shape[1]))
    return h


def context_table(input_ids, context_len):
    """repeat_scope="dialog": (ctx int32 [G, max c - 1], lengths int32 [G]) of the dialogs' context tokens input_ids[g, 1:c)."""
    c = torch.as_tensor(np.asarray(context_len), dtype=torch.int64).reshape(-1)
    w = max(int(c.max()) - 1, 1)
    ctx = input_ids[:, 1:1 + w].to(torch.int32)
    if ctx.shape[1] < w:
        ctx = torch.nn.functional.pad(ctx, (0, w - ctx.shape[1]))
    keep = torch.arange(w, device=ctx.device)[None] < (c.to(ctx.device) - 1)[:, None]
    return torch.where(keep, ctx, 0).contiguous(), (c - 1).to(torch.int32).to(ctx.device)


def sample_search(step, G, samples, limits, max_answer_len, min_answer_len=1, length_penalty=0.0, device="cpu", greedy=False):
    """Draw `samples` answers per dialog.  step(k, token, flags) -> (token int [G*samples], logp fp32, logq fp32): the draw of every
    slot at step k with its two log-probabilities, where slot s = g * samples + j continues itself with answer token k-1 =
    token[s] (k = 0: every slot of a dialog starts from the dialog's root; `token` is ignored).  flags as in beam_search
    (step_flags).  A slot is finished when it draws [SEP]: at its dialog's limit at the latest, which forces it.  Finished slots
    keep running through `step`; what they draw is dropped.  -> GeneratedAnswers with the samples in draw order j.
    greedy: every dialog has samples + 1 slots, s = g * (samples + 1) + j, and `step` decodes slot j = samples greedily (the first
    token of the rank order, its log p, log q = 0).  The loop runs until that slot has finished too; its answer is returned in
    `.greedy`, what beam_search(beams=1) returns: logp summed in step order, scores = logp / length ** length_penalty with the
    divisor beam_search uses, step_logq None."""
    if greedy and not samples:
        raise ValueError("generate_answers: greedy=True adds a greedy slot to a sampling call and needs samples >= 1; for greedy "
                         "decoding alone use beams=1")
    N, samples = int(samples), int(samples) + bool(greedy)
    S, W = G * samples, max_answer_len + 1
    dev = torch.device(device)
    limits = torch.as_tensor(np.asarray(limits), dtype=torch.int64).to(dev)
    toks = torch.zeros((S, W), dtype=torch.int64, device=dev)
    lp = torch.zeros((S, W), dtype=F32, device=dev)
    lq = torch.zeros((S, W), dtype=F32, device=dev)
    lengths = torch.zeros(S, dtype=torch.int64, device=dev)
    done = torch.zeros(S, dtype=torch.bool, device=dev)
    token = torch.zeros(S, dtype=torch.int64, device=dev)
    if greedy:                                                                # beam_search's arithmetic for the greedy slots
        gcum = torch.zeros(G, dtype=F32, device=dev)
        gscore = torch.full((G,), float("-inf"), dtype=F32, device=dev)
    for k in range(W):
        tok, p, q = step(k, token, step_flags(k, limits, samples, min_answer_len).to(dev))
        tok = tok.to(dev, torch.int64)
        live = ~done
        toks[:, k] = torch.where(live, tok, 0)
        lp[:, k] = torch.where(live, p.to(dev, F32), 0.0)
        lq[:, k] = torch.where(live, q.to(dev, F32), 0.0)
        fin = live & (tok == SEP)
        if greedy:
            gcum = gcum + lp[:, k].view(G, samples)[:, N]
            gscore = torch.where(fin.view(G, samples)[:, N], gcum / float((k + 1) ** length_penalty), gscore)
        lengths = torch.where(fin, k + 1, lengths)
        done = done | fin
        token = tok.clamp_min(0)
        if bool(done.all()):                                                  # the step's one device -> host synchronisation
            break
    lengths = lengths.view(G, samples)
    return sampled_answers(toks.view(G, samples, W), lp.view(G, samples, W), lq.view(G, samples, W), lengths, N, length_penalty,
                           (torch.where(lengths[:, N] > 0, gcum, float("-inf")), gscore) if greedy else None)


def sampled_answers(toks, lp, lq, lengths, N, length_penalty, greedy=None):
    """The result of a sampling call from its [G, N (+ 1), ...] tables: the N draws as the call without the greedy slot returns
    them (contiguous [G, N, ...]); greedy = (logp [G], scores [G]) of slot N, in beam_search's arithmetic -> `.greedy`, that slot
    on its own."""
    logp = lp.sum(2)
    scores = logp / lengths.clamp_min(1).to(F32) ** float(length_penalty)
    out = GeneratedAnswers(tokens=toks[:, :N].contiguous(), lengths=lengths[:, :N].contiguous(), scores=scores[:, :N].contiguous(),
                           logp=logp[:, :N].contiguous(), step_logp=lp[:, :N].contiguous(), step_logq=lq[:, :N].contiguous())
    if greedy is not None:
        out.greedy = GeneratedAnswers(tokens=toks[:, N:].contiguous(), lengths=lengths[:, N:].contiguous(),
                                      scores=greedy[1].view(-1, 1), logp=greedy[0].view(-1, 1), step_logp=lp[:, N:].contiguous())
    return out


def _greedy_sums(lp, lengths, W, length_penalty, dev):
    """beam_search's arithmetic of one slot per row: logp summed in step order in fp32, scores = logp / length ** penalty."""
    logp = torch.zeros(lp.shape[0], dtype=F32, device=dev)
    for k in range(W):
        logp = torch.where(lengths > k, logp + lp[:, k], logp)
    div = torch.tensor([float((k + 1) ** length_penalty) for k in range(W)], dtype=F32, device=dev)
    return logp, logp / div[lengths - 1]


# ---------------------------------------------------------------------------------------------------------------------------
# the engine's step function
# ---------------------------------------------------------------------------------------------------------------------------
def generate_answers(model, input_ids, image_feat, image_loc, context_len, token_type_ids=None, position_ids=None,
                     image_attention_mask=None, image_index=None, *, beams=1, max_answer_len=20, min_answer_len=1,
                     length_penalty=0.0, banned_tokens=(0, 101, 103), samples=0, temperature=1.0, top_k=0, top_p=1.0, seed=0,
                     sample_streams=None, greedy=False, no_repeat_ngram_size=0, repetition_penalty=1.0, repeat_scope="answer",
                     ensemble=None, ensemble_weights=None, ensemble_mode="prob", plausibility=0.0, draft_accept="match", draft=None,
                     draft_len=4):
    """BertForMultiModalPreTraining.generate_answers (see the module docstring) -> GeneratedAnswers on the model's device."""
    check_model(model)                                      # here, before the inputs are staged: nothing reaches the device
    G, T = input_ids.shape
    c_h = (context_len.cpu().numpy() if torch.is_tensor(context_len) else np.asarray(context_len)).astype(np.int64).reshape(-1)
    if c_h.shape[0] != G:
        raise ValueError(f"generate_answers: {c_h.shape[0]} context lengths for {G} dialogs")
    limits = check_request(c_h, T, beams, max_answer_len, min_answer_len)
    constraints = check_constraints(no_repeat_ngram_size, repetition_penalty, repeat_scope, beams)
    if constraints is not None and (int(limits.max()) > MAX_HISTORY or int(c_h.max()) - 1 > MAX_CONTEXT):
        raise ValueError(f"generate_answers: no_repeat_ngram_size / repetition_penalty keep a history of at most {MAX_HISTORY} answer "
                         f"and {MAX_CONTEXT} context tokens per hypothesis (got {int(limits.max())} and {int(c_h.max()) - 1})")
    if draft_accept not in ("match", "rejection"):
        raise ValueError(f"generate_answers: draft_accept must be 'match' or 'rejection', got {draft_accept!r}")
    if draft is None and draft_accept == "rejection":
        raise ValueError("generate_answers: draft_accept='rejection' is speculative sampling and needs a draft model (draft=...)")
    ensemble = check_ensemble(model, ensemble, ensemble_weights, ensemble_mode, plausibility, draft, no_repeat_ngram_size,
                              repetition_penalty)
    if draft is not None:                                   # speculative decoding: refused requests, still on the host
        from .speculative import check_draft
        draft = check_draft(model, draft, draft_len, beams, samples, no_repeat_ngram_size, repetition_penalty, repeat_scope,
                            draft_accept)
    sampling = None
    if greedy and not samples:
        raise ValueError("generate_answers: greedy=True adds a greedy slot to a sampling call and needs samples >= 1; for greedy "
                         "decoding alone use beams=1")
    if samples:
        ts, ks, ps, per_draw = check_sampling(samples, beams, temperature, top_k, top_p, greedy)
        streams = np.arange(G) if sample_streams is None else np.asarray(
            sample_streams.cpu() if torch.is_tensor(sample_streams) else sample_streams).astype(np.int64).reshape(-1)
        if streams.shape[0] != G:
            raise ValueError(f"generate_answers: {streams.shape[0]} sample streams for {G} dialogs")
        streams = streams[:, None] * int(samples) + np.arange(int(samples))[None]
        if greedy:                                         # the greedy slot keeps one id: its stream decides nothing
            streams = np.concatenate([streams, np.zeros((G, 1), dtype=np.int64)], 1)
        sampling = dict(samples=int(samples), greedy=bool(greedy), seed=int(seed),
                        streams=(streams.reshape(-1) & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
        if per_draw or greedy or constraints is not None or draft is not None:   # per-row parameters: unimm_lm_sample_rows (_hist
            # and the rejection step take no other form)
            sampling["rows"] = slot_parameters(G, ts, ks, ps, greedy)
        else:
            sampling.update(temperature=float(ts[0]), top_k=int(ks[0]), top_p=float(ps[0]))
    eng = model._engine
    eng.ensure(model._device())
    inp = dict(input_ids=input_ids, image_feat=image_feat, image_loc=image_loc, token_type_ids=token_type_ids,
               position_ids=position_ids, image_attention_mask=image_attention_mask, image_index=image_index)
    inp = {k: v for k, v in inp.items() if v is not None}
    eng.stage_host_inputs(inp, pack=("attention_mask", "co_attention_mask"))   # the [G, R] image key mask stays a tensor
    if draft is not None:
        from .speculative import speculate
        draft._engine.ensure(model._device())
        return eng._on_text_stream(speculate, eng, draft._engine, inp, c_h, limits, int(draft_len), max_answer_len, min_answer_len,
                                   length_penalty, tuple(int(t) for t in banned_tokens), sampling)
    if ensemble is not None:                                # every member decodes on an engine of its own
        ensemble["engines"] = [p._engine for p in ensemble["partners"]]
        for peng in ensemble["engines"]:
            peng.ensure(model._device())
    return eng._on_text_stream(_generate, eng, inp, c_h, limits, beams, max_answer_len, min_answer_len, length_penalty,
                               tuple(int(t) for t in banned_tokens), sampling, constraints, ensemble)


def _generate(eng, inp, c_h, limits, beams, max_answer_len, min_answer_len, length_penalty, banned_tokens, sampling=None,
              constraints=None, ensemble=None):
    """The engine's step functions.  `beams` below is the number of hypothesis slots per dialog: the beams, or the samples.
    ensemble (check_ensemble's dict with the partners' `engines`): one DecodeSide per member, stepped in lockstep on the same
    tokens; the selection launches then read the rows unimm_lm_mix makes of the members' logits."""
    if sampling is not None:
        beams = sampling["samples"] + sampling["greedy"]
    dev, V = eng.arena.device, eng.cfg.vocab_size
    pcap = max(int(limits.max()), 1)
    banned = torch.tensor(banned_tokens, dtype=torch.int32, device=dev) if banned_tokens else None
    side = DecodeSide(eng, inp, c_h, limits, pcap, banned, beams, beams)      # a dialog's slots are one attention group
    pre, G, S = side.pre, side.G, side.S
    vals = torch.empty((S, beams), dtype=F32, device=dev)
    tops = torch.empty((S, beams), dtype=torch.int32, device=dev)
    sides = [side]
    if ensemble is not None:                               # the partners: the same slots and groups, each on its own engine
        sides += [p._on_text_stream(DecodeSide, p, inp, c_h, limits, pcap, banned, beams, beams) for p in ensemble["engines"]]
        # the mixed rows: columns [V, Vpad) stay 0 and are never rewritten -- the mix writes, and the selection kernels read, [0, V)
        mixed = torch.zeros((S, pre["logits"].shape[1]), dtype=F32, device=dev)

    def on(s, fn, *args):
        """One entry of a side, a partner's on its engine's text stream (the model's, unless that engine keeps one of its own)."""
        return fn(*args) if s is side else s.eng._on_text_stream(fn, *args)

    def mix(blocks, rows, flags):
        from . import mix as MX                            # the extension library: loaded by the calls that mix
        MX.lm_mix([b[:rows] for b in blocks], ensemble["weights"], ensemble["mode"], V, banned, flags, SEP, ensemble["log_alpha"],
                  mixed[:rows])
        return mixed[:rows]

    def step_logits(token, k, flags):
        """The rows the selection reads at step k >= 1: answer row k-1 and copy row k of every slot through every member."""
        if ensemble is None:
            return side.rows(token[:, None], k, [0])
        return mix([on(s, s.rows, token[:, None], k, [0]) for s in sides], S, flags)

    if constraints is not None:                            # the history rules: every launch below is a _hist entry point
        answers = new_history(S, pcap, dev)
        ctx, ctx_len = context_table(inp["input_ids"].to(dev), c_h) if constraints["scope"] == "dialog" else (None, None)
        slot_ctx = torch.arange(S, device=dev, dtype=torch.int32) // beams if ctx is not None else None
        root_ctx = torch.arange(G, device=dev, dtype=torch.int32) if ctx is not None else None

        def history(root=False):
            """The launch's unimm_lm_history: of the S slots, or (root) of the G rows of the prefill, whose answers are empty."""
            return L.lm_history(answers["hist"], answers["len"], constraints["ngram"], constraints["penalty"], SEP, ctx, ctx_len,
                                root_ctx if root else slot_ctx)

    def topk(logits, rows, flags, k, parent=None, token=None):
        if constraints is None:
            L.lm_topk(logits, rows, V, banned, flags, SEP, beams, vals[:rows], tops[:rows])
        else:
            track_history(answers, k, token, parent)
            L.lm_topk_hist(logits, rows, V, banned, flags, SEP, beams, history(root=k == 0), vals[:rows], tops[:rows])

    def step(k, parent, token, flags):
        if k == 0:                                         # copy row 0 is the prefill's decoded row
            root = flags[::beams].contiguous()
            topk(pre["logits"] if ensemble is None else mix([s.pre["logits"] for s in sides], G, root), G, root, 0)
            return vals[:G].repeat_interleave(beams, 0), tops[:G].repeat_interleave(beams, 0)
        if k >= 2:                                         # children inherit their parent's cache + its answer row k-2
            for s in sides:
                on(s, s.reorder, parent)
        topk(step_logits(token, k, flags), S, flags, k, parent, token)        # answer row k-1 and copy row k of every slot
        return vals, tops

    if sampling is None:
        return beam_search(step, G, beams, limits, max_answer_len, min_answer_len, length_penalty, device=dev)

    streams = torch.from_numpy(sampling["streams"]).to(dev)
    stok = torch.empty(S, dtype=torch.int32, device=dev)
    slp = torch.empty(S, dtype=F32, device=dev)
    slq = torch.empty(S, dtype=F32, device=dev)

    rows = [torch.from_numpy(a).to(dev) for a in sampling["rows"]] if "rows" in sampling else None

    def draw(k, logits, flags, token=None):
        key = DR.make_key(sampling["seed"], k, SAMPLE_SITE)
        if constraints is not None:
            track_history(answers, k, token)
            L.lm_sample_hist(logits, S, V, banned, flags, SEP, rows[0], rows[1], rows[2], key, streams, history(), stok, slp, slq)
        elif rows is not None:
            L.lm_sample_rows(logits, S, V, banned, flags, SEP, rows[0], rows[1], rows[2], key, streams, stok, slp, slq)
        else:
            L.lm_sample(logits, S, V, banned, flags, SEP, sampling["temperature"], sampling["top_k"], sampling["top_p"], key,
                        streams, stok, slp, slq)
        return stok, slp, slq

    def sample_step(k, token, flags):
        if k == 0:                                         # every slot of a dialog draws from the prefill's copy row 0
            root = pre["logits"] if ensemble is None else mix([s.pre["logits"] for s in sides], G, flags[::beams].contiguous())
            return draw(k, root[:, :V].repeat_interleave(beams, 0), flags)
        if k >= 2:                                         # a slot keeps its own cache: append its answer row k-2 in place
            for s in sides:
                on(s, s.append_in_place, k - 2)
        return draw(k, step_logits(token, k, flags), flags, token)

    return sample_search(sample_step, G, sampling["samples"], limits, max_answer_len, min_answer_len, length_penalty, device=dev,
                         greedy=sampling["greedy"])
